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
// No atomics; every sum has a fixed order, so runs are bit-identical.
#pragma once

#include "common.h"
#include "heads_grad_plan.h"

namespace sfa {

typedef float hg_f32x16 __attribute__((ext_vector_type(16)));

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

// The level's fp16x3 weight terms [2][M][K] (model.hip split_terms_h3) cut into [2][Na][K] and [2][M - Na][K], the
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

}  // namespace sfa
