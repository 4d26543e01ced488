// Plan of sfa_model_neck_forward / sfa_model_neck_grad (neck.hip), plain C++ so that a host program can walk it
// (tools/neck_plan_check.cpp): the pixel and channel tiles of the pointwise GEMMs, the split-K chunks of the
// weight gradients, the per-block partials of the bias gradients and the workspace regions, built on grad_plan.h's
// tiles, split-K and bias records.  The entries and the workspace-size functions all go through
// neck_forward_plan() / neck_grad_plan().
//
// The neck (models/fpn_resnet.py:197-210) has four resolutions r = 0..3 of (2^r h4, 2^r w4) and three stages
// f = 1..3: stage f is a 1x1 convolution at resolution f with kNkCout[f-1] outputs over kNkUp[f-1] "up" input
// channels (the stage before, resized) and kNkSkip[f-1] skip channels (layer 4-f of the backbone).
#pragma once

#include <cstddef>
#include <cstdint>

#include "grad_plan.h"

namespace sfa {

constexpr int kNkMaxRows = 8191;  // h4: the resize kernel's grid holds 8 h4 rows

constexpr int kNkCout[3] = {256, 128, 64};
constexpr int kNkUp[3] = {512, 256, 128};
constexpr int kNkSkip[3] = {256, 128, 64};

// One weight-gradient GEMM: rows x cols of dW over the split-K's pixels.
struct NeckWgrad : GradSplitK {
  int rows, cols;
};

struct NeckForwardPlan {
  int npix[4];                             // B (2^r h4) (2^r w4)
  size_t off_up, off_z1, off_z2, total;    // bytes: U l4 (npix[1] x 512), z1 (npix[1] x 256), z2 (npix[2] x 128)
};

struct NeckGradPlan {
  int npix[4];
  NeckWgrad wg[4];  // dW1a (over l4, at resolution 0), dW1b (over l3), dW2, dW3
  GradBias bs[3];   // db1, db2, db3
  // bytes: d_u3 (npix[3] x 128), dZ2 (npix[2] x 128), d_u2 (npix[2] x 256), dZ1 (npix[1] x 256), dL (npix[0] x 256),
  // the float32 split-K partials (the largest of the four GEMMs: they run one after the other) and the float64
  // bias partials (the largest of the three)
  size_t off_du3, off_dz2, off_du2, off_dz1, off_dl, off_part, off_bpart, total;
};

// false: non-positive sizes, more rows than the resize kernel's grid holds, or a map whose byte offsets pass 31
// bits (the widest is 128 channels at resolution 3: B h4 w4 2^15 bytes).
inline bool neck_dims(int B, int h4, int w4, int npix[4]) {
  if (B <= 0 || h4 <= 0 || w4 <= 0 || h4 > kNkMaxRows) return false;
  const int64_t n0 = (int64_t)B * h4 * w4;
  if (n0 * 64 * 128 * 4 >= ((int64_t)1 << 31)) return false;
  for (int r = 0; r < 4; ++r) npix[r] = (int)(n0 << (2 * r));
  return true;
}

inline bool neck_forward_plan(int B, int h4, int w4, NeckForwardPlan* p) {
  if (!neck_dims(B, h4, w4, p->npix)) return false;
  GradRegions ws;
  p->off_up = ws.take((size_t)p->npix[1] * 512 * 4);
  p->off_z1 = ws.take((size_t)p->npix[1] * 256 * 4);
  p->off_z2 = ws.take((size_t)p->npix[2] * 128 * 4);
  p->total = ws.cur;
  return true;
}

inline bool neck_grad_plan(int B, int h4, int w4, int max_chunk_pixels, NeckGradPlan* p) {
  if (max_chunk_pixels < 0 || !neck_dims(B, h4, w4, p->npix)) return false;
  const int wrows[4] = {256, 256, 128, 64}, wcols[4] = {512, 256, 384, 192};
  size_t part = 0, bpart = 0;
  for (int i = 0; i < 4; ++i) {
    NeckWgrad& g = p->wg[i];
    static_cast<GradSplitK&>(g) = grad_split_k(p->npix[i], max_chunk_pixels);
    g.rows = wrows[i], g.cols = wcols[i];
    const size_t bytes = (size_t)g.chunks * g.rows * g.cols * 4;
    if (bytes > part) part = bytes;
  }
  for (int f = 0; f < 3; ++f) {
    p->bs[f] = grad_bias(p->npix[f + 1], kNkCout[f]);
    if (grad_bias_bytes(p->bs[f]) > bpart) bpart = grad_bias_bytes(p->bs[f]);
  }
  GradRegions ws;
  p->off_du3 = ws.take((size_t)p->npix[3] * 128 * 4);
  p->off_dz2 = ws.take((size_t)p->npix[2] * 128 * 4);
  p->off_du2 = ws.take((size_t)p->npix[2] * 256 * 4);
  p->off_dz1 = ws.take((size_t)p->npix[1] * 256 * 4);
  p->off_dl = ws.take((size_t)p->npix[0] * 256 * 4);
  p->off_part = ws.take(part);
  p->off_bpart = ws.take(bpart);
  p->total = ws.cur;
  return true;
}

}  // namespace sfa
