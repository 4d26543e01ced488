// Plan of sfa_model_heads_grad (heads_grad.hip), plain C++ so that a host program can walk it
// (tools/heads_grad_plan_check.cpp): the tiles of heads_wgrad_kernel, its split-K chunks, the per-block
// partials of heads_dhidden_kernel and the workspace regions.  The entry and
// sfa_model_heads_grad_workspace_size both go through heads_grad_plan().
//
// One level's heads: x (B, h, w, Cin) NHWC, M = 64 * heads hidden channels.  The weight gradient is an
// implicit GEMM with K = the pixels; K is cut into chunks of whole rows of one frame (never crossing a
// frame), every chunk writes its partial (M x 9 x Cin) tile and a fold adds the chunks in chunk order.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SFA_HG_HD __host__ __device__
#else
#define SFA_HG_HD
#endif

namespace sfa {

constexpr int kHgTile = 64;           // hidden channels and input channels of one workgroup (2 x 2 waves of 32 x 32)
constexpr int kHgSeg = 32;            // pixels of one row staged in LDS per step (16 MFMA k-steps)
constexpr int kHgChunkPixels = 4096;  // the plan's own chunk size (max_chunk_pixels == 0), in pixels
constexpr int kHgDhMinPixels = 32;    // heads_dhidden_kernel: fewest pixels of one block ...
constexpr int kHgDhMaxBlocks = 1024;  // ... and most blocks (what its fold walks per element)
constexpr int kHgHidden = 64;         // head_conv
constexpr size_t kHgAlign = 256;      // workspace regions

struct HeadsGradChunk {
  int frame, row0, rows;
};

struct HeadsGradPlan {
  int B, h, w, Cin, heads, M;
  int rows_per_chunk, chunks_per_frame, num_chunks;
  int Kc;  // pixels of the largest chunk: the K of the longest float32 accumulation
  int dh_pixels, dh_blocks, dh_slots;  // pixels per block, blocks, float64 words per block
  // The hidden recompute runs the fp16x3 convolution once on the first Na columns (a multiple of 128) and once on
  // the last Nb (64 with an odd head count, else 0): the widths its standard-epilogue kernels take.  The hidden
  // region holds [pixels][Na] then [pixels][Nb]; the terms region holds the level's fp16 terms cut the same way,
  // [2][Na][K] then [2][Nb][K] (K = 9 Cin); the amax region holds the per-frame max |x| words of x.
  int Na, Nb;
  size_t off_hidden, off_dhidden, off_part, off_dpart, off_terms, off_amax, total;  // bytes
};

constexpr int kHgAmaxWords = 256;  // words of one frame's max |x| record (conv.h SFA_AMAX_WORDS)

inline size_t hg_align_up(size_t v) { return (v + kHgAlign - 1) / kHgAlign * kHgAlign; }

// false: a shape outside the kernels' range (non-positive size, Cin not a multiple of the tile, heads outside
// 1..8, negative max_chunk_pixels, or a map whose byte offsets pass 31 bits).
inline bool heads_grad_plan(int B, int h, int w, int Cin, int heads, int max_chunk_pixels, HeadsGradPlan* p) {
  if (B <= 0 || h <= 0 || w <= 0 || Cin <= 0 || Cin % kHgTile != 0 || heads < 1 || heads > 8 ||
      max_chunk_pixels < 0)
    return false;
  const int M = kHgHidden * heads;
  const int64_t npix = (int64_t)B * h * w;
  const int64_t widest = Cin > M ? Cin : M;
  if (npix * widest * 4 >= ((int64_t)1 << 31)) return false;
  p->B = B, p->h = h, p->w = w, p->Cin = Cin, p->heads = heads, p->M = M;
  const int cap = max_chunk_pixels > 0 ? max_chunk_pixels : kHgChunkPixels;
  int rows = cap / w;
  if (rows < 1) rows = 1;  // a chunk is at least one whole row
  if (rows > h) rows = h;
  p->rows_per_chunk = rows;
  p->chunks_per_frame = (h + rows - 1) / rows;
  p->num_chunks = B * p->chunks_per_frame;
  p->Kc = rows * w;
  int dp = (int)((npix + kHgDhMaxBlocks - 1) / kHgDhMaxBlocks);
  if (dp < kHgDhMinPixels) dp = kHgDhMinPixels;
  p->dh_pixels = dp;
  p->dh_blocks = (int)((npix + dp - 1) / dp);
  p->dh_slots = M * 5 + heads * 4;  // per hidden channel dW2[0..3], db1; per head db2[0..3]
  size_t cur = 0;
  auto take = [&](size_t bytes) {
    const size_t o = cur;
    cur = hg_align_up(cur + bytes);
    return o;
  };
  p->off_hidden = take((size_t)npix * M * 4);
  p->off_dhidden = take((size_t)npix * M * 4);
  p->off_part = take((size_t)p->num_chunks * M * 9 * Cin * 4);
  p->off_dpart = take((size_t)p->dh_blocks * p->dh_slots * 8);
  p->Na = heads / 2 * 128;
  p->Nb = heads % 2 * 64;
  p->off_terms = take((size_t)2 * M * 9 * Cin * 2);
  p->off_amax = take((size_t)B * kHgAmaxWords * 4);
  p->total = cur;
  return true;
}

// Chunk c, 0 <= c < num_chunks: frame-major, then rows.  heads_wgrad_kernel calls this very function.
SFA_HG_HD inline HeadsGradChunk heads_grad_chunk_at(int c, int h, int rows_per_chunk, int chunks_per_frame) {
  HeadsGradChunk k;
  k.frame = c / chunks_per_frame;
  k.row0 = (c - k.frame * chunks_per_frame) * rows_per_chunk;
  k.rows = h - k.row0 < rows_per_chunk ? h - k.row0 : rows_per_chunk;
  return k;
}

inline HeadsGradChunk heads_grad_chunk(const HeadsGradPlan& p, int c) {
  return heads_grad_chunk_at(c, p.h, p.rows_per_chunk, p.chunks_per_frame);
}

}  // namespace sfa
