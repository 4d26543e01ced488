// Plan of sfa_model_heads_grad (heads_grad.hip), plain C++ so that a host program can walk it
// (tools/heads_grad_plan_check.cpp): the tiles of heads_wgrad_kernel, its split-K chunks, the per-block
// partials of heads_dhidden_kernel and the workspace regions.  The entry and
// sfa_model_heads_grad_workspace_size both go through heads_grad_plan().  Below it the tiling of
// heads_dgrad_kernel (sfa_model_heads_input_grad) and the workspace of sfa_model_heads_forward.
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
constexpr int kHgDgPix = 64;          // heads_dgrad_kernel: pixels of one image row per workgroup (2 x 2 waves of 32 x 32)
constexpr int kHgDgCin = 64;          // ... its input channels (level 2 has 64 in all)
constexpr int kHgDgSlice = 16;        // ... hidden channels staged in LDS per step (8 MFMA k-steps per tap)
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

// heads_dgrad_kernel: one workgroup owns kHgDgPix pixels of one image row and kHgDgCin input channels and walks
// the whole K = 9 M itself.  Workgroups are numbered channel tile first, then the row's pixel tiles, then the
// rows of all frames.
struct HeadsDgradTile {
  int row;     // frame * h + y
  int col0;    // first pixel of the tile in its row
  int cols;    // 1 .. kHgDgPix: the last tile of a row may be short
  int chan0;   // first input channel
};

struct HeadsDgradPlan {
  int tiles_per_row, chan_tiles;
  int64_t blocks;  // tiles_per_row * chan_tiles * B * h
};

// false: as heads_grad_plan (the same shapes and the same 31-bit byte-offset limit), or more blocks than one
// grid dimension holds.
inline bool heads_dgrad_plan(int B, int h, int w, int Cin, int heads, HeadsDgradPlan* p) {
  HeadsGradPlan g;
  if (Cin % kHgDgCin != 0 || !heads_grad_plan(B, h, w, Cin, heads, 0, &g)) return false;
  p->tiles_per_row = (w + kHgDgPix - 1) / kHgDgPix;
  p->chan_tiles = Cin / kHgDgCin;
  p->blocks = (int64_t)p->tiles_per_row * p->chan_tiles * B * h;
  return p->blocks < ((int64_t)1 << 31);
}

// Block c, 0 <= c < blocks.  heads_dgrad_kernel calls this very function.
SFA_HG_HD inline HeadsDgradTile heads_dgrad_tile_at(int c, int w, int tiles_per_row, int chan_tiles) {
  HeadsDgradTile t;
  const int ct = c % chan_tiles, rest = c / chan_tiles;
  const int pt = rest % tiles_per_row;
  t.row = rest / tiles_per_row;
  t.col0 = pt * kHgDgPix;
  t.cols = w - t.col0 < kHgDgPix ? w - t.col0 : kHgDgPix;
  t.chan0 = ct * kHgDgCin;
  return t;
}

// Workspace of sfa_model_heads_forward: the hidden activation in the two column parts the fp16x3 convolutions
// write ([pixels][Na] then [pixels][Nb], as in HeadsGradPlan), the cut fp16 terms and the frames' max |x| records.
struct HeadsForwardPlan {
  int M, Na, Nb;
  size_t off_hidden, off_terms, off_amax, total;  // bytes
};

inline bool heads_forward_plan(int B, int h, int w, int Cin, int heads, HeadsForwardPlan* p) {
  HeadsGradPlan g;
  if (!heads_grad_plan(B, h, w, Cin, heads, 0, &g)) return false;
  p->M = g.M, p->Na = g.Na, p->Nb = g.Nb;
  const size_t npix = (size_t)B * h * w;
  p->off_hidden = 0;
  p->off_terms = hg_align_up(npix * g.M * 4);
  p->off_amax = p->off_terms + hg_align_up((size_t)2 * g.M * 9 * Cin * 2);
  p->total = p->off_amax + hg_align_up((size_t)B * kHgAmaxWords * 4);
  return true;
}

}  // namespace sfa
