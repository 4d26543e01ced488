// Plan of sfa_model_neck_forward / sfa_model_neck_grad (neck.hip), plain C++ so that a host program can walk it
// (tools/neck_plan_check.cpp): the pixel and channel tiles of the pointwise GEMMs, the split-K chunks of the
// weight gradients, the per-block partials of the bias gradients and the workspace regions.  The entries and the
// workspace-size functions all go through neck_forward_plan() / neck_grad_plan().
//
// The neck (models/fpn_resnet.py:197-210) has four resolutions r = 0..3 of (2^r h4, 2^r w4) and three stages
// f = 1..3: stage f is a 1x1 convolution at resolution f with kNkCout[f-1] outputs over kNkUp[f-1] "up" input
// channels (the stage before, resized) and kNkSkip[f-1] skip channels (layer 4-f of the backbone).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SFA_NK_HD __host__ __device__
#else
#define SFA_NK_HD
#endif

namespace sfa {

constexpr int kNkTile = 64;            // pixels (or output channels) and channels of one workgroup (2 x 2 waves of 32 x 32)
constexpr int kNkStep = 16;            // K of one LDS step (8 MFMA k-steps)
constexpr int kNkChunkPixels = 2048;   // the plan's own split-K chunk (max_chunk_pixels == 0), in pixels
constexpr int kNkBiasMinPixels = 64;   // neck_bias_kernel: fewest pixels of one block ...
constexpr int kNkBiasMaxBlocks = 256;  // ... and most blocks (what its fold walks per channel)
constexpr int kNkMaxRows = 8191;       // h4: the resize kernel's grid holds 8 h4 rows
constexpr size_t kNkAlign = 256;       // workspace regions

constexpr int kNkCout[3] = {256, 128, 64};
constexpr int kNkUp[3] = {512, 256, 128};
constexpr int kNkSkip[3] = {256, 128, 64};

struct NeckRange {
  int first, count;
};

// One weight-gradient GEMM: rows x cols of dW over npix pixels in chunks of Kc (the last may be short).
struct NeckWgrad {
  int rows, cols, npix, Kc, chunks;
};

// One bias gradient: blocks of `pixels` consecutive pixels (the last may be short), cout float64 words each.
struct NeckBias {
  int npix, cout, pixels, blocks;
};

struct NeckForwardPlan {
  int npix[4];                             // B (2^r h4) (2^r w4)
  size_t off_up, off_z1, off_z2, total;    // bytes: U l4 (npix[1] x 512), z1 (npix[1] x 256), z2 (npix[2] x 128)
};

struct NeckGradPlan {
  int npix[4];
  NeckWgrad wg[4];  // dW1a (over l4, at resolution 0), dW1b (over l3), dW2, dW3
  NeckBias bs[3];   // db1, db2, db3
  // bytes: d_u3 (npix[3] x 128), dZ2 (npix[2] x 128), d_u2 (npix[2] x 256), dZ1 (npix[1] x 256), dL (npix[0] x 256),
  // the float32 split-K partials (the largest of the four GEMMs: they run one after the other) and the float64
  // bias partials (the largest of the three)
  size_t off_du3, off_dz2, off_du2, off_dz1, off_dl, off_part, off_bpart, total;
};

inline size_t nk_align_up(size_t v) { return (v + kNkAlign - 1) / kNkAlign * kNkAlign; }

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
  p->off_up = 0;
  p->off_z1 = nk_align_up((size_t)p->npix[1] * 512 * 4);
  p->off_z2 = p->off_z1 + nk_align_up((size_t)p->npix[1] * 256 * 4);
  p->total = p->off_z2 + nk_align_up((size_t)p->npix[2] * 128 * 4);
  return true;
}

inline bool neck_grad_plan(int B, int h4, int w4, int max_chunk_pixels, NeckGradPlan* p) {
  if (max_chunk_pixels < 0 || !neck_dims(B, h4, w4, p->npix)) return false;
  const int cap = max_chunk_pixels > 0 ? max_chunk_pixels : kNkChunkPixels;
  const int wrows[4] = {256, 256, 128, 64}, wcols[4] = {512, 256, 384, 192}, wres[4] = {0, 1, 2, 3};
  size_t part = 0, bpart = 0;
  for (int i = 0; i < 4; ++i) {
    NeckWgrad& g = p->wg[i];
    g.rows = wrows[i], g.cols = wcols[i], g.npix = p->npix[wres[i]];
    g.Kc = g.npix < cap ? g.npix : cap;
    g.chunks = (g.npix + g.Kc - 1) / g.Kc;
    const size_t bytes = (size_t)g.chunks * g.rows * g.cols * 4;
    if (bytes > part) part = bytes;
  }
  for (int f = 0; f < 3; ++f) {
    NeckBias& b = p->bs[f];
    b.npix = p->npix[f + 1], b.cout = kNkCout[f];
    int px = (b.npix + kNkBiasMaxBlocks - 1) / kNkBiasMaxBlocks;
    if (px < kNkBiasMinPixels) px = kNkBiasMinPixels;
    b.pixels = px;
    b.blocks = (b.npix + px - 1) / px;
    const size_t bytes = (size_t)b.blocks * b.cout * 8;
    if (bytes > bpart) bpart = bytes;
  }
  size_t cur = 0;
  auto take = [&](size_t bytes) {
    const size_t o = cur;
    cur = nk_align_up(cur + bytes);
    return o;
  };
  p->off_du3 = take((size_t)p->npix[3] * 128 * 4);
  p->off_dz2 = take((size_t)p->npix[2] * 128 * 4);
  p->off_du2 = take((size_t)p->npix[2] * 256 * 4);
  p->off_dz1 = take((size_t)p->npix[1] * 256 * 4);
  p->off_dl = take((size_t)p->npix[0] * 256 * 4);
  p->off_part = take(part);
  p->off_bpart = take(bpart);
  p->total = cur;
  return true;
}

// Tiles of kNkTile over n items (pixels of a map, channels of a matrix): tile t of neck_tiles(n).  The kernels
// call these very functions.
SFA_NK_HD inline int neck_tiles(int n) { return (n + kNkTile - 1) / kNkTile; }
SFA_NK_HD inline NeckRange neck_tile_at(int t, int n) {
  NeckRange r;
  r.first = t * kNkTile;
  r.count = n - r.first < kNkTile ? n - r.first : kNkTile;
  return r;
}

// Chunk c of a split of n pixels into runs of `per` (split-K chunks with per = Kc, bias blocks with per = pixels).
SFA_NK_HD inline NeckRange neck_chunk_at(int c, int n, int per) {
  NeckRange r;
  r.first = c * per;
  r.count = n - r.first < per ? n - r.first : per;
  return r;
}

}  // namespace sfa
