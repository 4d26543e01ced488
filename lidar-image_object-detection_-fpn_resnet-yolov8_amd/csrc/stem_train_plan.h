// Plan of sfa_stem_train_forward / sfa_stem_train_grad (stem_train.hip), plain C++ so that a host program can walk it
// (tools/stem_train_plan_check.cpp): the stem (models/fpn_resnet.py:179-182) with bn1 in training mode (batch
// statistics), on stem_grad_plan.h's shape and source functions, block_train_plan.h's statistics blocks and
// grad_plan.h's split-K and regions.  The entries and the size functions all go through stem_train_forward_plan() /
// stem_train_grad_plan().
//
// n = B oh ow, the values one channel of bn1 sees; a plan refuses n < 2 as block_train_plan.h does.
#pragma once

#include "block_train_plan.h"
#include "stem_grad_plan.h"

namespace sfa {

constexpr int kStK = kSgK;             // 147 (c, ky, kx) entries of conv1's K, in torch's order (stem_column)
constexpr int kStKPad = 160;           // ... padded to whole LDS steps of kGradStep: rows 147..159 of the k-major W are zero
constexpr int kStWpLd = 49 * 4;        // words of one row of the [o][tap][4] copy stem_dgrad_kernel reads
// Size limits of the launches this operator makes (all index in 32 bits below a map of 2^31 bytes):
//   B <= 65535 and ph <= 65535 (the max-pool puts the frame and the pooled row on grid axes), so H <= 4 * 65535.
// W has no limit of its own.  The fp16x3 convolution's 16-bit row / column packing (kSgMaxSide) does not apply here.
constexpr int kStMaxBatch = 65535;
constexpr int kStMaxH = 4 * 65535;

static_assert(kStKPad % kGradStep == 0 && kStKPad >= kStK, "conv1's K in whole steps");

struct StemTrainForwardPlan {
  StemShape s;
  GradBias st;  // the statistics blocks
  // bytes: the k-major copy [k][64] of W (kStKPad rows), the float64 partials [block][64][2] of the statistics, and
  // the float32 (s, t) pair [2][64] the apply launch reads
  size_t off_wk, off_spart, off_coef, total;
};

struct StemTrainGradPlan {
  StemShape s;
  BlockWgrad wg;  // dW: rows 64, cin 147, taps 1 (as StemGradPlan)
  GradBias st;    // the blocks of the backward's two sums
  // bytes: dY and dZ (npix_a x 64 each), the [o][tap][4] copy of W the data gradient reads, the float32 split-K
  // partials [chunk][64][147], the float64 partials [block][64][2] of the reduction and its folded sums [64][2]
  size_t off_dy, off_dz, off_wp, off_part, off_rpart, off_sums, total;
};

// 0: fine; 1: outside the arguments' domain (non-positive sizes, a map of 2^31 bytes or more: x read as 16 bytes per
// pixel bounds the image as in stem_shape(), a is the largest map); 2: a size the launches cannot index.
inline int stem_train_shape(int B, int H, int W, StemShape* s) {
  if (B <= 0 || H <= 0 || W <= 0) return 1;
  if (B > kStMaxBatch || H > kStMaxH) return 2;
  s->B = B, s->H = H, s->W = W;
  s->oh = (H + 1) / 2, s->ow = (W + 1) / 2;
  s->ph = (s->oh + 1) / 2, s->pw = (s->ow + 1) / 2;
  const int64_t nx = (int64_t)B * H * W, na = (int64_t)B * s->oh * s->ow, np = (int64_t)B * s->ph * s->pw;
  const int64_t lim = (int64_t)1 << 31;
  if (nx * 16 >= lim || na * kSgC * 4 >= lim) return 1;
  s->npix_x = (int)nx, s->npix_a = (int)na, s->npix_p = (int)np;
  return 0;
}

inline bool stem_train_forward_plan(int B, int H, int W, int max_chunk_pixels, StemTrainForwardPlan* p) {
  if (max_chunk_pixels < 0 || stem_train_shape(B, H, W, &p->s) != 0 || p->s.npix_a < 2) return false;
  p->st = block_train_stat_blocks(p->s.npix_a, kSgC, max_chunk_pixels);
  GradRegions ws;
  p->off_wk = ws.take((size_t)kStKPad * kSgC * 4);
  p->off_spart = ws.take((size_t)p->st.blocks * kSgC * 16);
  p->off_coef = ws.take((size_t)2 * kSgC * 4);
  p->total = ws.cur;
  return true;
}

inline bool stem_train_grad_plan(int B, int H, int W, int max_chunk_pixels, StemTrainGradPlan* p) {
  if (max_chunk_pixels < 0 || stem_train_shape(B, H, W, &p->s) != 0 || p->s.npix_a < 2) return false;
  const StemShape& s = p->s;
  BlockWgrad& g = p->wg;
  static_cast<GradSplitK&>(g) = grad_split_k(s.npix_a, max_chunk_pixels);
  g.rows = kSgC, g.cin = kSgK, g.taps = 1;
  p->st = block_train_stat_blocks(s.npix_a, kSgC, max_chunk_pixels);
  const size_t map = (size_t)s.npix_a * kSgC * 4;
  GradRegions ws;
  p->off_dy = ws.take(map);
  p->off_dz = ws.take(map);
  p->off_wp = ws.take((size_t)kSgC * kStWpLd * 4);
  p->off_part = ws.take((size_t)g.chunks * kSgC * kSgK * 4);
  p->off_rpart = ws.take((size_t)p->st.blocks * kSgC * 16);
  p->off_sums = ws.take((size_t)kSgC * 16);
  p->total = ws.cur;
  return true;
}

}  // namespace sfa
