// Plan of sfa_model_stem_forward / sfa_model_stem_grad (stem_grad.hip), plain C++ so that a host program can walk it
// (tools/stem_grad_plan_check.cpp): the sizes of the stem's maps, the window / tap source functions the kernels and
// the host check share, the split-K chunks of dW', the per-block partials of db' and the workspace regions.  The
// entries and the workspace-size functions all go through stem_forward_plan() / stem_grad_plan().
//
// Stem (models/fpn_resnet.py:179-182): x (B, 3, H, W) NCHW -> conv 7x7 / 2 / pad 3 + folded bn1 + ReLU ->
// a (B, oh, ow, 64) NHWC, oh = ceil(H / 2), ow = ceil(W / 2) -> MaxPool2d(3, 2, 1) -> p (B, ph, pw, 64),
// ph = ceil(oh / 2), pw = ceil(ow / 2).
#pragma once

#include <cstddef>
#include <cstdint>

#include "block_plan.h"

namespace sfa {

constexpr int kSgC = 64;              // the stem's output channels
constexpr int kSgK = 147;             // 3 x 7 x 7: the columns of dW' in torch's (c, ky, kx) order
constexpr int kSgColTiles = 3;        // 147 columns padded to 3 tiles of kGradTile
constexpr int kSgMaxSide = 32760;     // the forward's conv launch packs input rows and columns in 16 bits
constexpr int kSgMaxBatch = 65535;    // the forward's layout and max-pool launches put the frame on a grid axis
constexpr int kSgDgradPixels = 256;   // image pixels of one stem_dgrad_kernel pass (one per thread)
constexpr int kSgDgradMaxBlocks = 2048;

struct StemShape {
  int B, H, W, oh, ow, ph, pw;
  int npix_x, npix_a, npix_p;  // B H W, B oh ow, B ph pw
};

struct StemForwardPlan {
  StemShape s;
  // bytes: x as (B, H, W, 4) for the model's conv launch, and its per-frame max |x| record
  size_t off_xin, off_amax, amax_bytes, total;
};

struct StemGradPlan {
  StemShape s;
  BlockWgrad wg;  // dW': rows 64, cin 147, taps 1 (the fold's (M, cin, ntaps) = torch's (64, 3 x 7 x 7))
  GradBias bs;    // db'
  // bytes: dA (npix_a x 64), the float32 split-K partials [chunk][64][147], the float64 bias partials
  size_t off_da, off_part, off_bpart, total;
};

// false: non-positive sizes, H or W above kSgMaxSide, B above kSgMaxBatch, or a map of 2^31 bytes or more (x as NHWC4 is the largest
// input form, a the largest map).
inline bool stem_shape(int B, int H, int W, StemShape* s) {
  if (B <= 0 || H <= 0 || W <= 0 || H > kSgMaxSide || W > kSgMaxSide || B > kSgMaxBatch) return false;
  s->B = B, s->H = H, s->W = W;
  s->oh = (H + 1) / 2, s->ow = (W + 1) / 2;
  s->ph = (s->oh + 1) / 2, s->pw = (s->ow + 1) / 2;
  const int64_t nx = (int64_t)B * H * W, na = (int64_t)B * s->oh * s->ow, np = (int64_t)B * s->ph * s->pw;
  const int64_t lim = (int64_t)1 << 31;
  if (nx * 16 >= lim || na * kSgC * 4 >= lim) return false;
  s->npix_x = (int)nx, s->npix_a = (int)na, s->npix_p = (int)np;
  return true;
}

inline bool stem_forward_plan(int B, int H, int W, StemForwardPlan* p) {
  if (!stem_shape(B, H, W, &p->s)) return false;
  GradRegions ws;
  p->off_xin = ws.take((size_t)p->s.npix_x * 16);
  p->amax_bytes = (size_t)B * SFA_AMAX_WORDS * 4;
  p->off_amax = ws.take(p->amax_bytes);
  p->total = ws.cur;
  return true;
}

inline bool stem_grad_plan(int B, int H, int W, int max_chunk_pixels, StemGradPlan* p) {
  if (max_chunk_pixels < 0 || !stem_shape(B, H, W, &p->s)) return false;
  const StemShape& s = p->s;
  BlockWgrad& g = p->wg;
  static_cast<GradSplitK&>(g) = grad_split_k(s.npix_a, max_chunk_pixels);
  g.rows = kSgC, g.cin = kSgK, g.taps = 1;
  p->bs = grad_bias(s.npix_a, kSgC);
  GradRegions ws;
  p->off_da = ws.take((size_t)s.npix_a * kSgC * 4);
  p->off_part = ws.take((size_t)g.chunks * kSgC * kSgK * 4);
  p->off_bpart = ws.take(grad_bias_bytes(p->bs));
  p->total = ws.cur;
  return true;
}

// ---- source functions, one axis at a time (rows and columns are independent); the kernels call these very functions

// The pool windows that hold conv-map index i (0 <= i < n; pn = ceil(n / 2) windows of 3 / stride 2 / pad 1, window
// v covering 2 v - 1 .. 2 v + 1): always v = i / 2, and at an odd i also i / 2 + 1 when that window exists.
SFA_GRAD_HD inline int stem_pool_first_window(int i) { return i >> 1; }
SFA_GRAD_HD inline int stem_pool_windows(int i, int pn) { return ((i & 1) && (i >> 1) + 1 < pn) ? 2 : 1; }

// The conv output index that image index i reaches through tap k of the 7-tap / pad 3 / stride 2 window:
// i = 2 o - 3 + k.  -1: none (wrong parity, or outside 0 .. on - 1).
SFA_GRAD_HD inline int stem_tap_source(int i, int k, int on) {
  const int t = i + 3 - k;
  if (t < 0 || (t & 1)) return -1;
  const int o = t >> 1;
  return o < on ? o : -1;
}

// The first tap of matching parity at image index i: the taps that can reach it are k0, k0 + 2, .. <= 6.
SFA_GRAD_HD inline int stem_first_tap(int i) { return (i + 3) & 1; }

// Column j of dW' (0 .. kSgK - 1, torch's order): input plane c and taps (ky, kx).
SFA_GRAD_HD inline void stem_column(int j, int* c, int* ky, int* kx) {
  *c = j / 49;
  const int r = j - *c * 49;
  *ky = r / 7;
  *kx = r - *ky * 7;
}

}  // namespace sfa
