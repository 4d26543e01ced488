// Plan of sfa_model_block_forward / sfa_model_block_grad (block.hip), plain C++ so that a host program can walk it
// (tools/block_plan_check.cpp): the shape of one BasicBlock, the pixel tiles of the data gradients, the split-K
// chunks of the weight gradients, the per-block partials of the bias gradients and the workspace regions, built on
// grad_plan.h's tiles, split-K and bias records.  The entries and the workspace-size functions all go through
// block_forward_plan() / block_grad_plan().
//
// Block layer{L}.{b} (models/fpn_resnet.py:42-71), L = 1..4, b = 0, 1: cout = 64 2^(L-1); cin = cout / 2 and
// stride 2 with a 1x1 stride-2 downsample for b == 0 && L > 1, else cin = cout, stride 1 and the identity skip.
// x is (B, h, w, cin); mid, y, gy are (B, oh, ow, cout) with oh = ceil(h / stride), ow = ceil(w / stride).
#pragma once

#include <cstddef>
#include <cstdint>

#include "conv_args.h"
#include "grad_plan.h"

namespace sfa {

struct BlockShape {
  int layer, block, B, h, w;
  int cin, cout, stride, downsample, oh, ow;
  int npix_in, npix_out;  // B h w, B oh ow
};

// One weight-gradient GEMM: rows x (taps cin) of dW over the split-K's output pixels.
struct BlockWgrad : GradSplitK {
  int rows, cin, taps;
};

struct BlockForwardPlan {
  BlockShape s;
  // bytes: the per-frame max |x| records of x and of mid, and the split-K partials of the 512-wide convolutions
  // (2 slices of (npix_out, cout); 0 bytes for narrower blocks)
  size_t off_amax_x, off_amax_mid, off_part, part_floats, total;
};

struct BlockGradPlan {
  BlockShape s;
  BlockWgrad wg[3];  // dW1' (over x, stride s), dW2' (over mid), dWd' (over x, the centre tap; taps = 0 without one)
  GradBias bs;       // db1', db2': the same geometry
  // bytes: dA (npix_out x cout), the float32 split-K partials (the largest of the GEMMs: they run one after the
  // other) and the float64 bias partials
  size_t off_da, off_part, off_bpart, total;
};

// false: layer or block out of range, non-positive sizes, or a map of 2^31 bytes or more.
inline bool block_shape(int layer, int block, int B, int h, int w, BlockShape* s) {
  if (layer < 1 || layer > 4 || block < 0 || block > 1 || B <= 0 || h <= 0 || w <= 0) return false;
  s->layer = layer, s->block = block, s->B = B, s->h = h, s->w = w;
  s->cout = 64 << (layer - 1);
  s->downsample = block == 0 && layer > 1;
  s->cin = s->downsample ? s->cout / 2 : s->cout;
  s->stride = s->downsample ? 2 : 1;
  s->oh = (h + s->stride - 1) / s->stride;
  s->ow = (w + s->stride - 1) / s->stride;
  const int64_t nin = (int64_t)B * h * w, nout = (int64_t)B * s->oh * s->ow;
  const int64_t lim = (int64_t)1 << 31;
  if (nin >= lim || nin * s->cin * 4 >= lim || nout * s->cout * 4 >= lim) return false;
  s->npix_in = (int)nin, s->npix_out = (int)nout;
  return true;
}

inline bool block_forward_plan(int layer, int block, int B, int h, int w, BlockForwardPlan* p) {
  if (!block_shape(layer, block, B, h, w, &p->s)) return false;
  GradRegions ws;
  p->off_amax_x = ws.take((size_t)B * SFA_AMAX_WORDS * 4);
  p->off_amax_mid = ws.take((size_t)B * SFA_AMAX_WORDS * 4);
  p->part_floats = p->s.cout >= 512 ? (size_t)2 * p->s.npix_out * p->s.cout : 0;
  p->off_part = ws.take(p->part_floats * 4);
  p->total = ws.cur;
  return true;
}

inline bool block_grad_plan(int layer, int block, int B, int h, int w, int max_chunk_pixels, BlockGradPlan* p) {
  if (max_chunk_pixels < 0 || !block_shape(layer, block, B, h, w, &p->s)) return false;
  const BlockShape& s = p->s;
  const int wcin[3] = {s.cin, s.cout, s.cin}, wtaps[3] = {9, 9, s.downsample ? 1 : 0};
  size_t part = 0;
  for (int i = 0; i < 3; ++i) {
    BlockWgrad& g = p->wg[i];
    static_cast<GradSplitK&>(g) = grad_split_k(s.npix_out, max_chunk_pixels);
    g.rows = s.cout, g.cin = wcin[i], g.taps = wtaps[i];
    const size_t bytes = (size_t)g.chunks * g.rows * g.taps * g.cin * 4;
    if (bytes > part) part = bytes;
  }
  p->bs = grad_bias(s.npix_out, s.cout);
  GradRegions ws;
  p->off_da = ws.take((size_t)s.npix_out * s.cout * 4);
  p->off_part = ws.take(part);
  p->off_bpart = ws.take(grad_bias_bytes(p->bs));
  p->total = ws.cur;
  return true;
}

// The output pixel (along one axis) that input index i reaches through tap k of a 3-tap / pad-1 / stride-s window:
// i = o s - 1 + k.  -1: none (between the strides, or outside 0 .. on - 1).
SFA_GRAD_HD inline int block_tap_source(int i, int k, int s, int on) {
  const int t = i + 1 - k;
  if (t < 0 || t % s != 0) return -1;
  const int o = t / s;
  return o < on ? o : -1;
}

// The kernels' arguments (block_kernel.h), here so that a host file can fill them (block_host.h).

// The maps of one data gradient.  g0 (B, oh, ow, cout), masked by m0 when it is not null, meets W0 [o][tap cin + c]
// (row stride ldw0) through the nine taps; g1 / m1 / W1 [o][c] (row stride ldw1), when g1 is not null, through the
// centre tap alone.  eg / em: the masked map the epilogue adds (same shape as out), or null.  om: the map whose sign
// masks the result, or null.
struct BkDgrad {
  const float *g0, *m0, *W0, *g1, *m1, *W1, *eg, *em, *om;
  int ldw0, ldw1;
  int h, w, oh, ow, s, cin, cout, npix;  // out is (B, h, w, cin), npix = B h w
};

// One weight gradient.  g (B, oh, ow, M) masked by gm when it is not null; x (B, h, w, cin) read through taps
// tap0 .. tap0 + ntaps - 1 of the 3x3 / pad 1 / stride s window.
struct BkWgrad {
  const float *g, *gm, *x;
  int h, w, oh, ow, s, cin, M, tap0, ntaps, npix, Kc;  // npix = B oh ow
};

}  // namespace sfa
