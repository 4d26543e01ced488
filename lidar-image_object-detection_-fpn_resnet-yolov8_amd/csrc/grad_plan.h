// What the plans of the float32-MFMA gradient operators share (neck_plan.h, block_plan.h, stem_grad_plan.h), plain
// C++ so that a host program can walk it (tools/plan_check.h): the 64-wide tiles, the split-K chunks of a weight
// gradient, the per-block partials of a bias gradient and the cursor that lays out workspace regions.  The kernels
// (grad_tile.h and the operators' own) call the very functions the plans and the host checks call.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SFA_GRAD_HD __host__ __device__
#else
#define SFA_GRAD_HD
#endif

namespace sfa {

constexpr int kGradTile = 64;            // pixels (or output channels) and channels of one workgroup (2 x 2 waves of 32 x 32)
constexpr int kGradStep = 16;            // K of one LDS step (8 MFMA k-steps)
constexpr int kGradChunkPixels = 2048;   // a plan's own split-K chunk (max_chunk_pixels == 0), in pixels
constexpr int kGradBiasMinPixels = 64;   // grad_bias_kernel: fewest pixels of one block ...
constexpr int kGradBiasMaxBlocks = 256;  // ... and most blocks (what its fold walks per channel)
constexpr size_t kGradAlign = 256;       // workspace regions

struct GradRange {
  int first, count;
};

// The split-K of one weight gradient: npix pixels in chunks of Kc (the last may be short).
struct GradSplitK {
  int npix, Kc, chunks;
};

// One bias gradient: blocks of `pixels` consecutive pixels (the last may be short), cout float64 words each.
struct GradBias {
  int npix, cout, pixels, blocks;
};

// npix > 0, max_chunk_pixels >= 0 (0: the plan's own chunk)
inline GradSplitK grad_split_k(int npix, int max_chunk_pixels) {
  const int cap = max_chunk_pixels > 0 ? max_chunk_pixels : kGradChunkPixels;
  GradSplitK k;
  k.npix = npix;
  k.Kc = npix < cap ? npix : cap;
  k.chunks = (npix + k.Kc - 1) / k.Kc;
  return k;
}

inline GradBias grad_bias(int npix, int cout) {
  GradBias b;
  b.npix = npix, b.cout = cout;
  b.pixels = (npix + kGradBiasMaxBlocks - 1) / kGradBiasMaxBlocks;
  if (b.pixels < kGradBiasMinPixels) b.pixels = kGradBiasMinPixels;
  b.blocks = (npix + b.pixels - 1) / b.pixels;
  return b;
}

inline size_t grad_bias_bytes(const GradBias& b) { return (size_t)b.blocks * b.cout * 8; }

inline size_t grad_align_up(size_t v) { return (v + kGradAlign - 1) / kGradAlign * kGradAlign; }

// Lays workspace regions one after the other, each at a multiple of kGradAlign: take() is the region's offset, and
// `cur` after the last take() the size of the workspace.
struct GradRegions {
  size_t cur = 0;
  size_t take(size_t bytes) {
    const size_t o = cur;
    cur = grad_align_up(cur + bytes);
    return o;
  }
};

// Tiles of kGradTile over n items (pixels of a map, channels of a matrix): tile t of grad_tiles(n).
SFA_GRAD_HD inline int grad_tiles(int n) { return (n + kGradTile - 1) / kGradTile; }
SFA_GRAD_HD inline GradRange grad_tile_at(int t, int n) {
  GradRange r;
  r.first = t * kGradTile;
  r.count = n - r.first < kGradTile ? n - r.first : kGradTile;
  return r;
}

// Chunk c of a split of n pixels into runs of `per` (split-K chunks with per = Kc, bias blocks with per = pixels).
SFA_GRAD_HD inline GradRange grad_chunk_at(int c, int n, int per) {
  GradRange r;
  r.first = c * per;
  r.count = n - r.first < per ? n - r.first : per;
  return r;
}

}  // namespace sfa
