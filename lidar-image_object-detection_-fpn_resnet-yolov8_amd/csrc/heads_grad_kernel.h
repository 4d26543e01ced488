// Kernels of sfa_model_heads_grad (gfx950): the parameter gradients of one KFPN level's detection heads
// (models/fpn_resnet.py:135-143: conv3x3 -> ReLU -> conv1x1 per head) from d total / d y, with the hidden
// activation Hd recomputed by the entry.
//
//   heads_terms_cut_kernel, heads_amax_kernel   what the fp16x3 hidden recompute needs beside the packed weights: the
//                            level's fp16 terms cut at the column split, and the per-frame max |x| of a caller's x
//   heads_dhidden_kernel     per pixel and hidden channel o (head j = o / 64): dA = Hd > 0 ? sum_c W2[c][o] g[c] : 0
//                            in float64 from the float32 operands, rounded once; and the block's float64 partial
//                            sums of dW2 (g Hd), db2 (g) and db1 (the rounded dA) over its run of pixels, in
//                            pixel order
//   heads_dhidden_fold_kernel  one thread per partial word: the blocks added in block order, rounded once,
//                            written in torch's layouts
//   heads_wgrad_kernel       dW1 as an implicit GEMM on v_mfma_f32_32x32x2_f32: rows = hidden channels, columns
//                            = input channels of one tap, K = pixels.  Lane (r, k) of the MFMA takes dA[pixel
//                            k][o + r] and x[pixel k shifted by the tap][i + r]: the NHWC rows are the operands
//                            as they lie.  A workgroup (2 x 2 waves of 32 x 32) owns a 64 x 64 (o, i) tile of
//                            all nine taps over one K-chunk (whole rows of one frame): 9 x 16 accumulator
//                            registers per lane; per step it stages 32 pixels of dA and the 3 x 34 pixel window
//                            of x (zero outside the map) in LDS, then 16 k-steps x 9 MFMAs per wave
//   heads_wgrad_fold_kernel  per dW1 element: the chunks added in chunk order in float64, rounded once, written
//                            as (64, Cin, 3, 3) per head
//
//   heads_dgrad_kernel       dX, the heads' input gradient (sfa_model_heads_input_grad): an implicit GEMM on the same
//                            instruction with rows = pixels of one image row, columns = input channels and the
//                            whole K = (tap, o) inside one workgroup; described at the kernel
//   heads_out_kernel         y = W2 Hd + b2 of sfa_model_heads_forward, float64 from the float32 operands
//
// No atomics; every sum has a fixed order, so runs are bit-identical.
#pragma once

#include "common.h"
#include "heads_grad_plan.h"

namespace sfa {

typedef float hg_f32x16 __attribute__((ext_vector_type(16)));
typedef float hg_f32x4 __attribute__((ext_vector_type(4)));

// Per head of the level: g = d total / d y (B, ch, h, w) and the four gradient outputs in torch's layouts.
struct HgHeads {
  const float* g[SFA_MAX_HEADS];
  float* gw1[SFA_MAX_HEADS];  // (64, Cin, 3, 3)
  float* gb1[SFA_MAX_HEADS];  // (64)
  float* gw2[SFA_MAX_HEADS];  // (ch, 64)
  float* gb2[SFA_MAX_HEADS];  // (ch)
  int ch[SFA_MAX_HEADS];
  int num_heads;
};

// heads_out_kernel's table: per head the output map y (B, ch, h, w)
struct HoHeads {
  float* y[SFA_MAX_HEADS];
  int ch[SFA_MAX_HEADS];
  int num_heads;
};

// t.<field>[j] for a runtime j without indexing the by-value table (that would put it in scratch)
#define HG_PICK(dst, field, j)                  \
  do {                                          \
    _Pragma("unroll") for (int q_ = 0; q_ < SFA_MAX_HEADS; ++q_) \
      if (q_ == (j)) dst = t.field[q_];         \
  } while (0)

// grid (dh_blocks), block (M): thread o walks pixels [blockIdx * pixels, ...) of the flat (B, h, w) map.
// w2: the packed 1x1 weights [head][4][64]; part: dh_slots float64 words per block.
// HdA [pixels][Na], HdB [pixels][M - Na]: the two parts the hidden recompute wrote; Hd_out: null, or the caller's
// (B, h, w, M) copy of Hd.
__global__ void __launch_bounds__(512) heads_dhidden_kernel(HgHeads t, const float* __restrict__ HdA,
                                                            const float* __restrict__ HdB, int Na,
                                                            float* __restrict__ Hd_out,
                                                            const float* __restrict__ w2, float* __restrict__ dA,
                                                            double* __restrict__ part, int npix, int hw,
                                                            int pixels, int M) {
  const int o = threadIdx.x, j = o >> 6, k = o & 63;
  int ch = 0;
  const float* g = nullptr;
  HG_PICK(ch, ch, j);
  HG_PICK(g, g, j);
  double wv[4], s2[4], sg[4], s1 = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    wv[c] = c < ch ? (double)w2[(j * 4 + c) * 64 + k] : 0.0;
    s2[c] = sg[c] = 0.0;
  }
  const int p0 = (int)blockIdx.x * pixels;
  const int p1 = npix - p0 < pixels ? npix : p0 + pixels;
  for (int p = p0; p < p1; ++p) {
    const int b = p / hw, q = p - b * hw;
    const float hd = o < Na ? HdA[(size_t)p * Na + o] : HdB[(size_t)p * (M - Na) + (o - Na)];
    if (Hd_out) Hd_out[(size_t)p * M + o] = hd;
    double gv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) gv[c] = c < ch ? (double)g[((size_t)b * ch + c) * hw + q] : 0.0;
    double d = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) d += wv[c] * gv[c];
    const float da = hd > 0.f ? (float)d : 0.f;  // strict, as torch's ReLU backward
    dA[(size_t)p * M + o] = da;
    s1 += (double)da;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      s2[c] += gv[c] * (double)hd;
      sg[c] += gv[c];
    }
  }
  double* P = part + (size_t)blockIdx.x * (M * 5 + t.num_heads * 4);
#pragma unroll
  for (int c = 0; c < 4; ++c) P[o * 5 + c] = s2[c];
  P[o * 5 + 4] = s1;
  if (k == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) P[M * 5 + j * 4 + c] = sg[c];
  }
}

// The level's fp16x3 weight terms [2][M][K] (pack_row.h pack_fp16_terms) cut into [2][Na][K] and [2][M - Na][K], the
// form a convolution over those columns reads (its low terms follow its own high terms).  32-bit words, Kw = K / 2.
// grid (ceil(2 M Kw / 256)), block (256)
__global__ void __launch_bounds__(256) heads_terms_cut_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dstA,
                                                              uint32_t* __restrict__ dstB, int M, int Na, int Kw) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= 2 * M * Kw) return;
  const int term = e / (M * Kw), rem = e - term * (M * Kw);
  const int n = rem / Kw, k = rem - n * Kw;
  if (n < Na)
    dstA[((size_t)term * Na + n) * Kw + k] = src[e];
  else
    dstB[((size_t)term * (M - Na) + (n - Na)) * Kw + k] = src[e];
}

// max |x| of frame blockIdx.y, shard blockIdx.x of 8, into the frame's record (conv.h: a reader takes the max of the
// eight shard words, 32 words apart; no other word of the record is read).  n4 = float4s per frame.
// grid (8, B), block (256)
__global__ void __launch_bounds__(256) heads_amax_kernel(const float4* __restrict__ x, unsigned* __restrict__ amax, int n4) {
  __shared__ float red[4];
  const int per = (n4 + 7) / 8;
  const int lo = (int)blockIdx.x * per, hi = lo + per < n4 ? lo + per : n4;
  const float4* src = x + (size_t)blockIdx.y * n4;
  float m = 0.f;
  for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
    const float4 v = src[i];
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    amax[(size_t)blockIdx.y * kHgAmaxWords + blockIdx.x * 32] =
        __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

// grid (ceil(slots / 256)), block (256)
__global__ void __launch_bounds__(256) heads_dhidden_fold_kernel(HgHeads t, const double* __restrict__ part,
                                                                 int nblocks, int M) {
  const int slots = M * 5 + t.num_heads * 4;
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= slots) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * slots + e];
  const float r = (float)s;
  if (e < M * 5) {
    const int o = e / 5, c = e - o * 5, j = o >> 6, k = o & 63;
    int ch = 0;
    HG_PICK(ch, ch, j);
    if (c == 4) {
      float* dst = nullptr;
      HG_PICK(dst, gb1, j);
      dst[k] = r;
    } else if (c < ch) {
      float* dst = nullptr;
      HG_PICK(dst, gw2, j);
      dst[c * 64 + k] = r;
    }
  } else {
    const int e2 = e - M * 5, j = e2 >> 2, c = e2 & 3;
    int ch = 0;
    HG_PICK(ch, ch, j);
    if (c < ch) {
      float* dst = nullptr;
      HG_PICK(dst, gb2, j);
      dst[c] = r;
    }
  }
}

// grid (num_chunks, Cin / 64, M / 64), block (256).  part: [chunk][o][tap][i] float32.
__global__ void __launch_bounds__(256, 2) heads_wgrad_kernel(const float* __restrict__ dA, const float* __restrict__ x,
                                                             float* __restrict__ part, int h, int w, int Cin, int M,
                                                             int rows_per_chunk, int chunks_per_frame) {
  constexpr int S = kHgSeg, T = kHgTile, XW = S + 2;
  __shared__ __attribute__((aligned(16))) float sA[S * T];       // [pixel][o]
  __shared__ __attribute__((aligned(16))) float sX[3 * XW * T];  // [row y - 1 .. y + 1][column c0 - 1 ..][i]
  const int chunk = blockIdx.x, i0 = (int)blockIdx.y * T, o0 = (int)blockIdx.z * T;
  const HeadsGradChunk ck = heads_grad_chunk_at(chunk, h, rows_per_chunk, chunks_per_frame);
  const int b = ck.frame, row0 = ck.row0, rows = ck.rows;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wo = wave & 1, wi = wave >> 1, r = lane & 31, hh = lane >> 5;

  hg_f32x16 acc[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[tap][v] = 0.f;

  for (int y = row0; y < row0 + rows; ++y) {
    for (int c0 = 0; c0 < w; c0 += S) {
      const int sl = w - c0 < S ? w - c0 : S;
      __syncthreads();  // the previous step's fragment reads are done
      for (int e = tid; e < S * (T / 4); e += 256) {
        const int p = e >> 4, q4 = e & 15;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < sl) v = *reinterpret_cast<const float4*>(dA + ((size_t)((b * h + y) * w + c0 + p)) * M + o0 + q4 * 4);
        *reinterpret_cast<float4*>(sA + p * T + q4 * 4) = v;
      }
      for (int e = tid; e < 3 * XW * (T / 4); e += 256) {
        const int q4 = e & 15, pc = e >> 4;
        const int dy = pc / XW, col = pc - dy * XW;
        const int yy = y + dy - 1, xx = c0 + col - 1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w && col <= sl + 1)
          v = *reinterpret_cast<const float4*>(x + ((size_t)((b * h + yy) * w + xx)) * Cin + i0 + q4 * 4);
        *reinterpret_cast<float4*>(sX + pc * T + q4 * 4) = v;
      }
      __syncthreads();
      const int ks = (sl + 1) >> 1;  // an odd tail pairs with a zero row of sA
      for (int s = 0; s < ks; ++s) {
        const int p = 2 * s + hh;
        const float av = sA[p * T + wo * 32 + r];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int dy = tap / 3, dx = tap - dy * 3;
          const float bv = sX[(dy * XW + p + dx) * T + wi * 32 + r];
          acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[tap], 0, 0, 0);
        }
      }
    }
  }
  float* P = part + (size_t)chunk * M * 9 * Cin;
  const int i = i0 + wi * 32 + r;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int o = o0 + wo * 32 + (v & 3) + 8 * (v >> 2) + 4 * hh;
      P[((size_t)o * 9 + tap) * Cin + i] = acc[tap][v];
    }
}

// grid (ceil(M Cin 9 / 256)), block (256): element e = (o, i, tap) in the output's own order
__global__ void __launch_bounds__(256) heads_wgrad_fold_kernel(HgHeads t, const float* __restrict__ part, int nchunks,
                                                               int Cin, int M) {
  const int per_o = Cin * 9;
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= M * per_o) return;
  const int o = e / per_o, rem = e - o * per_o;
  const int i = rem / 9, tap = rem - i * 9;
  const size_t stride = (size_t)M * per_o;
  const float* src = part + ((size_t)o * 9 + tap) * Cin + i;
  double s = 0.0;
  for (int c = 0; c < nchunks; ++c) s += (double)src[(size_t)c * stride];
  float* dst = nullptr;
  HG_PICK(dst, gw1, o >> 6);
  dst[(size_t)(o & 63) * per_o + rem] = (float)s;
}

// The heads' input gradient dX[b,y,x,i] = sum_o sum_{ky,kx} dA[b, y+1-ky, x+1-kx, o] W1[o,i,ky,kx] (dA zero outside
// the map) as an implicit GEMM on v_mfma_f32_32x32x2_f32: rows = kHgDgPix pixels of one image row, columns =
// kHgDgCin input channels, K = (o, tap) = 9 M, all of it walked by this one workgroup (2 x 2 waves of 32 x 32, one
// 16-register accumulator each): no split-K, no partials, every element of dX written once by one lane.  Lane (r, k)
// takes dA[pixel r shifted by the flipped tap][o + k] and W1[o + k][tap][i + r]; w3 is [o][tap = ky * 3 + kx][i]
// (pack_plan.h PACK_CONV), so the W1 rows are the B operand as they lie.  Per step of kHgDgSlice hidden channels the
// workgroup stages the 3 x (kHgDgPix + 2) pixel window of dA, transposed to [o][row][pixel] so that the 32 pixels
// of a half-wave read 32 consecutive words, and the W1 slice [o][tap][i]: 12,672 + 36,864 = 49,536 bytes of LDS.
// The next step's global loads are issued into registers before the step's 72 MFMAs per wave.
// grid (blocks of heads_dgrad_plan), block (256)
__global__ void __launch_bounds__(256, 2) heads_dgrad_kernel(const float* __restrict__ dA, const float* __restrict__ w3,
                                                             float* __restrict__ dX, int h, int w, int Cin, int M,
                                                             int tiles_per_row, int chan_tiles) {
  constexpr int P = kHgDgPix, C = kHgDgCin, OS = kHgDgSlice, XW = P + 2;
  constexpr int SA_O = 3 * XW;                // words of one hidden channel's window
  constexpr int NA4 = 3 * XW * (OS / 4);      // float4 loads of one window slice
  constexpr int NW4 = OS * 9 * (C / 4);       // float4 loads of one weight slice
  constexpr int LA = (NA4 + 255) / 256, LW = NW4 / 256;
  static_assert(NW4 % 256 == 0 && OS % 4 == 0 && C == 64 && P == 64, "the staging loops assume these");
  __shared__ __attribute__((aligned(16))) float sA[OS * SA_O];    // [o][row y - 1 .. y + 1][column c0 - 1 ..]
  __shared__ __attribute__((aligned(16))) float sW[OS * 9 * C];   // [o][tap][i]
  const HeadsDgradTile tl = heads_dgrad_tile_at((int)blockIdx.x, w, tiles_per_row, chan_tiles);
  const int b = tl.row / h, y = tl.row - b * h, c0 = tl.col0, i0 = tl.chan0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave & 1, wc = wave >> 1, r = lane & 31, hh = lane >> 5;

  // where this thread's staging loads come from (-1: zero, outside the map) and go to
  int a_src[LA], a_dst[LA];
#pragma unroll
  for (int k = 0; k < LA; ++k) {
    const int e = tid + k * 256;
    const int q4 = e & (OS / 4 - 1), pc = e / (OS / 4);
    const int dy = pc / XW, col = pc - dy * XW;
    const int yy = y + dy - 1, xx = c0 + col - 1;
    const bool in = e < NA4 && (unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w;
    a_src[k] = in ? ((b * h + yy) * w + xx) * M + q4 * 4 : -1;  // < 2^29 words: the plan's offset limit
    a_dst[k] = e < NA4 ? (q4 * 4) * SA_O + pc : -1;
  }
  hg_f32x4 ra[LA], rw[LW];
  const float* wsrc = w3 + (size_t)(tid >> 4) * Cin + i0 + (tid & 15) * 4;  // e = tid + 256 k: row o * 9 + tap = e / 16
#define HG_DG_LOAD(o_first)                                                                                       \
  do {                                                                                                            \
    _Pragma("unroll") for (int k = 0; k < LA; ++k) ra[k] =                                                        \
        a_src[k] >= 0 ? *reinterpret_cast<const hg_f32x4*>(dA + (size_t)a_src[k] + (o_first)) : hg_f32x4{0.f, 0.f, 0.f, 0.f}; \
    _Pragma("unroll") for (int k = 0; k < LW; ++k) rw[k] =                                                        \
        *reinterpret_cast<const hg_f32x4*>(wsrc + ((size_t)(o_first) * 9 + k * 16) * Cin);                        \
  } while (0)

  hg_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  const bool live = wp * 32 < tl.cols;  // a short last tile: the waves of an empty pixel half only stage
  const int p = wp * 32 + r;

  HG_DG_LOAD(0);
  for (int o0 = 0; o0 < M; o0 += OS) {
    __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
    for (int k = 0; k < LA; ++k)
      if (a_dst[k] >= 0) {
        float* d = sA + a_dst[k];
        d[0] = ra[k].x, d[SA_O] = ra[k].y, d[2 * SA_O] = ra[k].z, d[3 * SA_O] = ra[k].w;
      }
#pragma unroll
    for (int k = 0; k < LW; ++k) *reinterpret_cast<hg_f32x4*>(sW + (tid + k * 256) * 4) = rw[k];
    __syncthreads();
    const int o_next = o0 + OS < M ? o0 + OS : o0;  // the last step loads its own slice again and drops it
    HG_DG_LOAD(o_next);
    if (live) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const float* A = sA + (2 - ky) * XW + p + 2 - kx + hh * SA_O;  // row y + 1 - ky, column c0 + p + 1 - kx
        const float* Wt = sW + tap * C + wc * 32 + r + hh * 9 * C;
#pragma unroll
        for (int s = 0; s < OS / 2; ++s)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[2 * s * SA_O], Wt[2 * s * 9 * C], acc, 0, 0, 0);
      }
    }
  }
#undef HG_DG_LOAD
  if (!live) return;
  float* out = dX + ((size_t)tl.row * w + c0) * Cin + i0 + wc * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = wp * 32 + (v & 3) + 8 * (v >> 2) + 4 * hh;
    if (q < tl.cols) out[(size_t)q * Cin] = acc[v];
  }
}

// y = W2 Hd + b2 of every head of the level: one thread per pixel and output slot (head j, channel c < 4), the 64
// products added to b2 in hidden-channel order in float64 from the float32 operands, rounded once, written NCHW per
// head.  HdA / HdB: the two column parts of the hidden recompute; Hd_out: null, or the joined (B, h, w, M) copy,
// written by the threads of slot c = 0.  w2: the packed 1x1 weights [head][4][64], b2: [head][4].
// grid (ceil(npix heads 4 / 256)), block (256)
__global__ void __launch_bounds__(256) heads_out_kernel(HoHeads t, const float* __restrict__ HdA,
                                                        const float* __restrict__ HdB, int Na, int M,
                                                        float* __restrict__ Hd_out, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, int npix, int hw) {
  const int slots = t.num_heads * 4;
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;  // < 2^29: the plan's offset limit
  if (e >= npix * slots) return;
  const int p = e / slots, slot = e - p * slots, j = slot >> 2, c = slot & 3;
  int ch = 0;
  HG_PICK(ch, ch, j);
  if (c >= ch && !(c == 0 && Hd_out)) return;
  const int o0 = j * 64;
  const float* hd = o0 < Na ? HdA + (size_t)p * Na + o0 : HdB + (size_t)p * (M - Na) + (o0 - Na);
  const float* wr = w2 + (j * 4 + c) * 64;
  double s = (double)b2[j * 4 + c];
  for (int k = 0; k < 64; k += 4) {
    const float4 hv = *reinterpret_cast<const float4*>(hd + k);
    const float4 wv = *reinterpret_cast<const float4*>(wr + k);
    s += (double)wv.x * (double)hv.x;
    s += (double)wv.y * (double)hv.y;
    s += (double)wv.z * (double)hv.z;
    s += (double)wv.w * (double)hv.w;
    if (c == 0 && Hd_out) *reinterpret_cast<float4*>(Hd_out + (size_t)p * M + o0 + k) = hv;
  }
  if (c >= ch) return;
  float* y = nullptr;
  HG_PICK(y, y, j);
  const int bb = p / hw, q = p - bb * hw;
  y[((size_t)bb * ch + c) * hw + q] = (float)s;
}

}  // namespace sfa
