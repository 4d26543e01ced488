// Plan of sfa_block_train_forward / sfa_block_train_grad (block_train.hip), plain C++ so that a host program can walk
// it (tools/block_train_plan_check.cpp): one BasicBlock of layer1..4 with its BatchNorms in training mode (batch
// statistics), on block_plan.h's shape and grad_plan.h's tiles, split-K and regions.  The entries and the size
// functions all go through block_train_forward_plan() / block_train_grad_plan().
//
// n = B oh ow, the values one channel of a BatchNorm sees; a plan refuses n < 2 (torch: "Expected more than 1 value
// per channel when training"; the running variance n / (n - 1) var does not exist).
#pragma once

#include "block_plan.h"

namespace sfa {

// The blocks of one per-channel float64 reduction over the n pixels of a map (the batch statistics, and the two sums
// of a BatchNorm's backward): grad_bias()'s blocks, which max_chunk_pixels > 0 shortens as far as
// kGradBiasMaxBlocks blocks allow, so that a small map is reduced through several partials.
inline GradBias block_train_stat_blocks(int npix, int cout, int max_chunk_pixels) {
  GradBias b = grad_bias(npix, cout);
  if (max_chunk_pixels > 0 && max_chunk_pixels < b.pixels) {
    const int least = (npix + kGradBiasMaxBlocks - 1) / kGradBiasMaxBlocks;
    b.pixels = max_chunk_pixels > least ? max_chunk_pixels : least;
    b.blocks = (npix + b.pixels - 1) / b.pixels;
  }
  return b;
}

struct BlockTrainForwardPlan {
  BlockShape s;
  int nbn;      // BatchNorms: 2, 3 with a downsample
  GradBias st;  // the statistics blocks
  // bytes: the k-major copies [tap cin + c][o] of W1, W2 and Wd (0 bytes without one), the float64 partials
  // [block][cout][2] of one BatchNorm's statistics (they run one after the other), and the float32 (s, t) pairs
  // [nbn][2][cout] the apply launches read
  size_t off_wk[3], wk_floats[3], off_spart, off_coef, total;
};

struct BlockTrainGradPlan {
  BlockShape s;
  int nbn;
  BlockWgrad wg[3];  // dW1 (over x, stride s), dW2 (over mid), dWd (over x, the centre tap; taps = 0 without one)
  GradBias st;       // the blocks of the backward's two sums
  // bytes: dZ2, dZd (0 bytes without a downsample), dA and dZ1 (npix_out x cout each), the [o][tap cin + c] copies
  // of W1 and W2 the data gradients read, the float32 split-K partials (the largest of the GEMMs), the float64
  // partials [block][cout][2] of one reduction and its folded sums [cout][2]
  size_t off_dz2, off_dzd, off_da, off_dz1, off_wt[2], wt_floats[2], off_part, off_rpart, off_sums, total;
};

inline bool block_train_forward_plan(int layer, int block, int B, int h, int w, int max_chunk_pixels,
                                     BlockTrainForwardPlan* p) {
  if (max_chunk_pixels < 0 || !block_shape(layer, block, B, h, w, &p->s) || p->s.npix_out < 2) return false;
  const BlockShape& s = p->s;
  p->nbn = s.downsample ? 3 : 2;
  p->st = block_train_stat_blocks(s.npix_out, s.cout, max_chunk_pixels);
  p->wk_floats[0] = (size_t)9 * s.cin * s.cout;
  p->wk_floats[1] = (size_t)9 * s.cout * s.cout;
  p->wk_floats[2] = s.downsample ? (size_t)s.cin * s.cout : 0;
  GradRegions ws;
  for (int i = 0; i < 3; ++i) p->off_wk[i] = ws.take(p->wk_floats[i] * 4);
  p->off_spart = ws.take((size_t)p->st.blocks * s.cout * 16);
  p->off_coef = ws.take((size_t)p->nbn * 2 * s.cout * 4);
  p->total = ws.cur;
  return true;
}

inline bool block_train_grad_plan(int layer, int block, int B, int h, int w, int max_chunk_pixels,
                                  BlockTrainGradPlan* p) {
  if (max_chunk_pixels < 0 || !block_shape(layer, block, B, h, w, &p->s) || p->s.npix_out < 2) return false;
  const BlockShape& s = p->s;
  p->nbn = s.downsample ? 3 : 2;
  const int wcin[3] = {s.cin, s.cout, s.cin}, wtaps[3] = {9, 9, s.downsample ? 1 : 0};
  size_t part = 0;
  for (int i = 0; i < 3; ++i) {
    BlockWgrad& g = p->wg[i];
    static_cast<GradSplitK&>(g) = grad_split_k(s.npix_out, max_chunk_pixels);
    g.rows = s.cout, g.cin = wcin[i], g.taps = wtaps[i];
    const size_t bytes = (size_t)g.chunks * g.rows * g.taps * g.cin * 4;
    if (bytes > part) part = bytes;
  }
  p->st = block_train_stat_blocks(s.npix_out, s.cout, max_chunk_pixels);
  const size_t map = (size_t)s.npix_out * s.cout * 4;
  p->wt_floats[0] = (size_t)9 * s.cin * s.cout;
  p->wt_floats[1] = (size_t)9 * s.cout * s.cout;
  GradRegions ws;
  p->off_dz2 = ws.take(map);
  p->off_dzd = ws.take(s.downsample ? map : 0);
  p->off_da = ws.take(map);
  p->off_dz1 = ws.take(map);
  for (int i = 0; i < 2; ++i) p->off_wt[i] = ws.take(p->wt_floats[i] * 4);
  p->off_part = ws.take(part);
  p->off_rpart = ws.take((size_t)p->st.blocks * s.cout * 16);
  p->off_sums = ws.take((size_t)s.cout * 16);
  p->total = ws.cur;
  return true;
}

// The input index (along one axis of n cells) that output index o reads through tap k of a 3-tap / pad-1 / stride-s
// window: i = o s - 1 + k.  -1: the padding.  The inverse of block_tap_source().
SFA_GRAD_HD inline int block_train_tap_input(int o, int k, int s, int n) {
  const int i = o * s - 1 + k;
  return (i >= 0 && i < n) ? i : -1;
}

}  // namespace sfa
