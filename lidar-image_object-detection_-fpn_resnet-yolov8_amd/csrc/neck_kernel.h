// Kernels of sfa_model_neck_forward / sfa_model_neck_grad (gfx950): the FPN neck of models/fpn_resnet.py:197-210,
// three 1x1 convolutions with bias over cat(up(x), skip) and three bilinear x2 resizes, and its gradients.
//
// One pointwise-GEMM family on v_mfma_f32_32x32x2_f32, a workgroup of 2 x 2 waves owning a 64 x 64 tile with one
// 16-register accumulator per wave, K walked in steps of kNkStep through two LDS tiles held k-major ([k][64],
// rows kNkLd words apart) so that lane (r, k) of the MFMA reads word r of row k for both operands.  The next
// step's global loads are issued into registers before the step's 8 MFMAs.  Three roles:
//   neck_fwd_kernel     rows = flat pixels, columns = Cout, K = the input channels read as two segments (the
//                       resized map, then the skip map: no concat buffer); bias in the epilogue
//   neck_dgrad_kernel   rows = flat pixels, columns = the input channels of one segment, K = Cout, all of it
//                       inside one workgroup; the epilogue adds the gradient that arrives at the same map from
//                       its own heads (g3 / g2) when there is one; every element stored once by one lane
//   neck_wgrad_kernel   rows = Cout, columns = input channels, K = the pixels of one split-K chunk: the NHWC rows
//                       of dZ and of the input maps are the operands as they lie; float32 partial tile per chunk
//   neck_wgrad_fold_kernel   per dW element: the chunks added in chunk order in float64, rounded once
//   neck_bias_kernel, neck_bias_fold_kernel   db: float64 sums over runs of pixels in pixel order, then over the
//                       runs in run order, rounded once
//   bilinear_up2_adjoint_kernel   U^T: per low-resolution element the float64 sum, in (row, column) order, of
//                       the high-resolution elements whose footprint reaches it times the float32 coefficients
//                       upsample2x_bilinear_kernel computes for that pixel (same expressions, same clamps)
//
// No atomics; every sum has a fixed order, so runs are bit-identical.
#pragma once

#include "common.h"
#include "neck_plan.h"

namespace sfa {

typedef float nk_f32x16 __attribute__((ext_vector_type(16)));
typedef float nk_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNkLd = kNkTile + 4;  // words between two k rows of an LDS tile: the transposing stores of a wave
                                    // (4 k-quads x 16 rows) then fall on 64 different banks
constexpr int kNkLdsWords = kNkStep * kNkLd;

// 64 rows x kNkStep k of an operand whose rows are K-contiguous (row stride ld words): thread t loads the float4 at
// row t / 4, k-quad t % 4 (zero at and past `rows`) and stores it transposed.
__device__ __forceinline__ nk_f32x4 nk_load_kc(const float* base, int ld, int row0, int rows, int k0, int tid) {
  const int m = tid >> 2, q4 = tid & 3;
  if (m >= rows) return nk_f32x4{0.f, 0.f, 0.f, 0.f};
  return *reinterpret_cast<const nk_f32x4*>(base + (size_t)(row0 + m) * ld + k0 + q4 * 4);
}
__device__ __forceinline__ void nk_store_kc(float* s, nk_f32x4 v, int tid) {
  float* d = s + (tid & 3) * 4 * kNkLd + (tid >> 2);
  d[0] = v.x, d[kNkLd] = v.y, d[2 * kNkLd] = v.z, d[3 * kNkLd] = v.w;
}

// kNkStep k x 64 columns of an operand that lies k-major (k row stride ld words): thread t loads the float4 at k row
// t / 16, column quad t % 16 (zero at and past `ks`) and stores it as it is.
__device__ __forceinline__ nk_f32x4 nk_load_mc(const float* base, int ld, int k0, int ks, int col0, int tid) {
  const int kk = tid >> 4, q4 = tid & 15;
  if (kk >= ks) return nk_f32x4{0.f, 0.f, 0.f, 0.f};
  return *reinterpret_cast<const nk_f32x4*>(base + (size_t)(k0 + kk) * ld + col0 + q4 * 4);
}
__device__ __forceinline__ void nk_store_mc(float* s, nk_f32x4 v, int tid) {
  *reinterpret_cast<nk_f32x4*>(s + (tid >> 4) * kNkLd + (tid & 15) * 4) = v;
}

// the step's 8 MFMAs of wave (wm, wn): rows wm * 32 .. of sA, columns wn * 32 .. of sB
__device__ __forceinline__ void nk_mma(const float* sA, const float* sB, int wm, int wn, int r, int hh, nk_f32x16& acc) {
  const float* A = sA + hh * kNkLd + wm * 32 + r;
  const float* Bp = sB + hh * kNkLd + wn * 32 + r;
#pragma unroll
  for (int s = 0; s < kNkStep / 2; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[2 * s * kNkLd], Bp[2 * s * kNkLd], acc, 0, 0, 0);
}

// row of accumulator register v inside the wave's 32 x 32 tile (the column is the lane's r)
__device__ __forceinline__ int nk_acc_row(int v, int hh) { return (v & 3) + 8 * (v >> 2) + 4 * hh; }

#define NK_LANE_IDS                                                 \
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;    \
  const int wm = wave & 1, wn = wave >> 1, r = lane & 31, hh = lane >> 5

// out[p][n] = bias[n] + sum_k cat(a0[p][0..k0), a1[p][0..k1))[k] W[n][k].  W: (N, k0 + k1) as torch keeps it.
// grid (neck_tiles(npix), N / 64), block (256)
__global__ void __launch_bounds__(256) neck_fwd_kernel(const float* __restrict__ a0, const float* __restrict__ a1,
                                                       int k0, int k1, const float* __restrict__ W,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       int npix, int N) {
  __shared__ __attribute__((aligned(16))) float sA[kNkLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kNkLdsWords];
  NK_LANE_IDS;
  const NeckRange pt = neck_tile_at((int)blockIdx.x, npix);
  const int n0 = (int)blockIdx.y * kNkTile, K = k0 + k1;
  auto load_a = [&](int k) {
    return k < k0 ? nk_load_kc(a0, k0, pt.first, pt.count, k, tid) : nk_load_kc(a1, k1, pt.first, pt.count, k - k0, tid);
  };
  nk_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  nk_f32x4 ra = load_a(0), rb = nk_load_kc(W, K, n0, kNkTile, 0, tid);
  for (int k = 0; k < K; k += kNkStep) {
    __syncthreads();  // the previous step's fragment reads are done
    nk_store_kc(sA, ra, tid);
    nk_store_kc(sB, rb, tid);
    __syncthreads();
    if (k + kNkStep < K) {
      ra = load_a(k + kNkStep);
      rb = nk_load_kc(W, K, n0, kNkTile, k + kNkStep, tid);
    }
    nk_mma(sA, sB, wm, wn, r, hh, acc);
  }
  const int n = n0 + wn * 32 + r;
  const float bv = bias[n];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = wm * 32 + nk_acc_row(v, hh);
    if (q < pt.count) out[(size_t)(pt.first + q) * N + n] = acc[v] + bv;
  }
}

// out[p][i] = (g ? g[p][i] : 0) + sum_o dz[p][o] W[o][i], i < N: W points at the segment's first column of the
// (K, ldw) weight matrix.
// grid (neck_tiles(npix), N / 64), block (256)
__global__ void __launch_bounds__(256) neck_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ W,
                                                         int ldw, const float* __restrict__ g,
                                                         float* __restrict__ out, int npix, int N, int K) {
  __shared__ __attribute__((aligned(16))) float sA[kNkLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kNkLdsWords];
  NK_LANE_IDS;
  const NeckRange pt = neck_tile_at((int)blockIdx.x, npix);
  const int i0 = (int)blockIdx.y * kNkTile;
  nk_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  nk_f32x4 ra = nk_load_kc(dz, K, pt.first, pt.count, 0, tid), rb = nk_load_mc(W, ldw, 0, kNkStep, i0, tid);
  for (int k = 0; k < K; k += kNkStep) {
    __syncthreads();
    nk_store_kc(sA, ra, tid);
    nk_store_mc(sB, rb, tid);
    __syncthreads();
    if (k + kNkStep < K) {
      ra = nk_load_kc(dz, K, pt.first, pt.count, k + kNkStep, tid);
      rb = nk_load_mc(W, ldw, k + kNkStep, kNkStep, i0, tid);
    }
    nk_mma(sA, sB, wm, wn, r, hh, acc);
  }
  const int i = i0 + wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = wm * 32 + nk_acc_row(v, hh);
    if (q < pt.count) {
      const size_t at = (size_t)(pt.first + q) * N + i;
      out[at] = g ? g[at] + acc[v] : acc[v];
    }
  }
}

// part[chunk][o][i] = sum over the chunk's pixels p of dz[p][o] x[p][i], x = cat(x0 (n0 channels), x1 (n1)).
// grid (chunks, (n0 + n1) / 64, M / 64), block (256)
__global__ void __launch_bounds__(256) neck_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x0,
                                                         const float* __restrict__ x1, int n0, int n1,
                                                         float* __restrict__ part, int npix, int Kc, int M) {
  __shared__ __attribute__((aligned(16))) float sA[kNkLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kNkLdsWords];
  NK_LANE_IDS;
  const NeckRange ck = neck_chunk_at((int)blockIdx.x, npix, Kc);
  const int i0 = (int)blockIdx.y * kNkTile, o0 = (int)blockIdx.z * kNkTile, N = n0 + n1;
  const float* x = i0 < n0 ? x0 : x1;  // a 64-channel tile lies in one segment: both widths are multiples of 64
  const int ldx = i0 < n0 ? n0 : n1, c0 = i0 < n0 ? i0 : i0 - n0;
  nk_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  nk_f32x4 ra = nk_load_mc(dz, M, ck.first, ck.count, o0, tid), rb = nk_load_mc(x, ldx, ck.first, ck.count, c0, tid);
  for (int k = 0; k < ck.count; k += kNkStep) {
    __syncthreads();
    nk_store_mc(sA, ra, tid);
    nk_store_mc(sB, rb, tid);
    __syncthreads();
    if (k + kNkStep < ck.count) {
      const int left = ck.count - (k + kNkStep);  // a short last step pairs with zero rows
      ra = nk_load_mc(dz, M, ck.first + k + kNkStep, left, o0, tid);
      rb = nk_load_mc(x, ldx, ck.first + k + kNkStep, left, c0, tid);
    }
    nk_mma(sA, sB, wm, wn, r, hh, acc);
  }
  float* P = part + (size_t)blockIdx.x * M * N;
  const int i = i0 + wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) P[(size_t)(o0 + wm * 32 + nk_acc_row(v, hh)) * N + i] = acc[v];
}

// dW[o][col0 + i] (row stride ldo) = the chunks of part[chunk][o][i] added in chunk order.
// grid (ceil(M N / 256)), block (256)
__global__ void __launch_bounds__(256) neck_wgrad_fold_kernel(const float* __restrict__ part, int chunks, int M, int N,
                                                              float* __restrict__ dW, int ldo, int col0) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= M * N) return;
  const int o = e / N, i = e - o * N;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += (double)part[(size_t)c * M * N + e];
  dW[(size_t)o * ldo + col0 + i] = (float)s;
}

// grid (blocks), block (cout): thread o adds dz[p][o] over the block's run of pixels.  part: [block][cout].
__global__ void __launch_bounds__(256) neck_bias_kernel(const float* __restrict__ dz, double* __restrict__ part,
                                                        int npix, int pixels, int cout) {
  const NeckRange run = neck_chunk_at((int)blockIdx.x, npix, pixels);
  const int o = threadIdx.x;
  double s = 0.0;
  for (int p = run.first; p < run.first + run.count; ++p) s += (double)dz[(size_t)p * cout + o];
  part[(size_t)blockIdx.x * cout + o] = s;
}

// grid (1), block (cout)
__global__ void __launch_bounds__(256) neck_bias_fold_kernel(const double* __restrict__ part, int blocks, int cout,
                                                             float* __restrict__ db) {
  const int o = threadIdx.x;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[(size_t)b * cout + o];
  db[o] = (float)s;
}

// The float32 weight with which source index i of a map of n enters output index o of its x2 resize: exactly
// upsample2x_bilinear_kernel's expressions (scale * o in float32, the clamp of the second tap), the two taps added
// when they fall on the same source.  0: outside o's footprint.
__device__ __forceinline__ double nk_up_weight(int o, int i, int n, float scale) {
  const float f = scale * (float)o;
  const int i0 = (int)f;
  const int i1 = i0 + (i0 < n - 1 ? 1 : 0);
  const float l1 = f - (float)i0, l0 = 1.f - l1;
  return (i0 == i ? (double)l0 : 0.0) + (i1 == i ? (double)l1 : 0.0);
}

// dst (B, H, W, C) = U^T src, src (B, 2 H, 2 W, C): one thread per element quad.  With scale < 1 / 2 only outputs
// 2 i - 3 .. 2 i + 3 can reach source i (2 i - 2 .. 2 i + 2 in exact arithmetic, one more each side for the
// float32 rounding of scale * o); each is tested with the forward's own expressions.
// grid (ceil(B H W C4 / 256)), block (256)
__global__ void __launch_bounds__(256) bilinear_up2_adjoint_kernel(const float4* __restrict__ src,
                                                                   float4* __restrict__ dst, int B, int H, int W,
                                                                   int C4, float sh, float sw) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= B * H * W * C4) return;
  const int c = e % C4, t = e / C4;
  const int x = t % W, t2 = t / W;
  const int y = t2 % H, b = t2 / H;
  double wy[7], wx[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int oy = 2 * y - 3 + j, ox = 2 * x - 3 + j;
    wy[j] = (oy >= 0 && oy < 2 * H) ? nk_up_weight(oy, y, H, sh) : 0.0;
    wx[j] = (ox >= 0 && ox < 2 * W) ? nk_up_weight(ox, x, W, sw) : 0.0;
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    if (wy[j] == 0.0) continue;
    const float4* row = src + ((size_t)(b * 2 * H + 2 * y - 3 + j) * (2 * W)) * C4 + c;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      if (wx[i] == 0.0) continue;
      const float4 v = row[(size_t)(2 * x - 3 + i) * C4];
      const double cf = wy[j] * wx[i];
      s0 += cf * (double)v.x;
      s1 += cf * (double)v.y;
      s2 += cf * (double)v.z;
      s3 += cf * (double)v.w;
    }
  }
  dst[e] = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
}

#undef NK_LANE_IDS

}  // namespace sfa
