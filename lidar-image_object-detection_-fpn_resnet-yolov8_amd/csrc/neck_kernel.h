// Kernels of sfa_model_neck_forward / sfa_model_neck_grad (gfx950): the FPN neck of models/fpn_resnet.py:197-210,
// three 1x1 convolutions with bias over cat(up(x), skip) and three bilinear x2 resizes, and its gradients.
//
// One pointwise-GEMM family on grad_tile.h's 64 x 64 tile (v_mfma_f32_32x32x2_f32, 2 x 2 waves, K walked in steps of
// kGradStep through two k-major LDS tiles).  The next step's global loads are issued into registers before the
// step's 8 MFMAs.  Three roles:
//   neck_fwd_kernel     rows = flat pixels, columns = Cout, K = the input channels read as two segments (the
//                       resized map, then the skip map: no concat buffer); bias in the epilogue
//   neck_dgrad_kernel   rows = flat pixels, columns = the input channels of one segment, K = Cout, all of it
//                       inside one workgroup; the epilogue adds the gradient that arrives at the same map from
//                       its own heads (g3 / g2) when there is one; every element stored once by one lane
//   neck_wgrad_kernel   rows = Cout, columns = input channels, K = the pixels of one split-K chunk: the NHWC rows
//                       of dZ and of the input maps are the operands as they lie; float32 partial tile per chunk
//                       (grad_common.hip's fold adds the chunks and its bias pair computes db)
//   bilinear_up2_adjoint_kernel   U^T: per low-resolution element the float64 sum, in (row, column) order, of
//                       the high-resolution elements whose footprint reaches it times the float32 coefficients
//                       upsample2x_bilinear_kernel computes for that pixel (same expressions, same clamps)
//
// No atomics; every sum has a fixed order, so runs are bit-identical.
#pragma once

#include "grad_tile.h"
#include "neck_plan.h"

namespace sfa {

// out[p][n] = bias[n] + sum_k cat(a0[p][0..k0), a1[p][0..k1))[k] W[n][k].  W: (N, k0 + k1) as torch keeps it.
// grid (grad_tiles(npix), N / 64), block (256)
__global__ void __launch_bounds__(256) neck_fwd_kernel(const float* __restrict__ a0, const float* __restrict__ a1,
                                                       int k0, int k1, const float* __restrict__ W,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       int npix, int N) {
  __shared__ __attribute__((aligned(16))) float sA[kGradLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kGradLdsWords];
  GRAD_LANE_IDS;
  const GradRange pt = grad_tile_at((int)blockIdx.x, npix);
  const int n0 = (int)blockIdx.y * kGradTile, K = k0 + k1;
  auto load_a = [&](int k) {
    return k < k0 ? grad_load_kc(a0, k0, pt.first, pt.count, k, tid) : grad_load_kc(a1, k1, pt.first, pt.count, k - k0, tid);
  };
  grad_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  grad_f32x4 ra = load_a(0), rb = grad_load_kc(W, K, n0, kGradTile, 0, tid);
  for (int k = 0; k < K; k += kGradStep) {
    __syncthreads();  // the previous step's fragment reads are done
    grad_store_kc(sA, ra, tid);
    grad_store_kc(sB, rb, tid);
    __syncthreads();
    if (k + kGradStep < K) {
      ra = load_a(k + kGradStep);
      rb = grad_load_kc(W, K, n0, kGradTile, k + kGradStep, tid);
    }
    grad_mma(sA, sB, wm, wn, r, hh, acc);
  }
  const int n = n0 + wn * 32 + r;
  const float bv = bias[n];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = wm * 32 + grad_acc_row(v, hh);
    if (q < pt.count) out[(size_t)(pt.first + q) * N + n] = acc[v] + bv;
  }
}

// out[p][i] = (g ? g[p][i] : 0) + sum_o dz[p][o] W[o][i], i < N: W points at the segment's first column of the
// (K, ldw) weight matrix.
// grid (grad_tiles(npix), N / 64), block (256)
__global__ void __launch_bounds__(256) neck_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ W,
                                                         int ldw, const float* __restrict__ g,
                                                         float* __restrict__ out, int npix, int N, int K) {
  __shared__ __attribute__((aligned(16))) float sA[kGradLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kGradLdsWords];
  GRAD_LANE_IDS;
  const GradRange pt = grad_tile_at((int)blockIdx.x, npix);
  const int i0 = (int)blockIdx.y * kGradTile;
  grad_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  grad_f32x4 ra = grad_load_kc(dz, K, pt.first, pt.count, 0, tid), rb = grad_load_mc(W, ldw, 0, kGradStep, i0, tid);
  for (int k = 0; k < K; k += kGradStep) {
    __syncthreads();
    grad_store_kc(sA, ra, tid);
    grad_store_mc(sB, rb, tid);
    __syncthreads();
    if (k + kGradStep < K) {
      ra = grad_load_kc(dz, K, pt.first, pt.count, k + kGradStep, tid);
      rb = grad_load_mc(W, ldw, k + kGradStep, kGradStep, i0, tid);
    }
    grad_mma(sA, sB, wm, wn, r, hh, acc);
  }
  const int i = i0 + wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = wm * 32 + grad_acc_row(v, hh);
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
  __shared__ __attribute__((aligned(16))) float sA[kGradLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kGradLdsWords];
  GRAD_LANE_IDS;
  const GradRange ck = grad_chunk_at((int)blockIdx.x, npix, Kc);
  const int i0 = (int)blockIdx.y * kGradTile, o0 = (int)blockIdx.z * kGradTile, N = n0 + n1;
  const float* x = i0 < n0 ? x0 : x1;  // a 64-channel tile lies in one segment: both widths are multiples of 64
  const int ldx = i0 < n0 ? n0 : n1, c0 = i0 < n0 ? i0 : i0 - n0;
  grad_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  grad_f32x4 ra = grad_load_mc(dz, M, ck.first, ck.count, o0, tid), rb = grad_load_mc(x, ldx, ck.first, ck.count, c0, tid);
  for (int k = 0; k < ck.count; k += kGradStep) {
    __syncthreads();
    grad_store_mc(sA, ra, tid);
    grad_store_mc(sB, rb, tid);
    __syncthreads();
    if (k + kGradStep < ck.count) {
      const int left = ck.count - (k + kGradStep);  // a short last step pairs with zero rows
      ra = grad_load_mc(dz, M, ck.first + k + kGradStep, left, o0, tid);
      rb = grad_load_mc(x, ldx, ck.first + k + kGradStep, left, c0, tid);
    }
    grad_mma(sA, sB, wm, wn, r, hh, acc);
  }
  float* P = part + (size_t)blockIdx.x * M * N;
  const int i = i0 + wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) P[(size_t)(o0 + wm * 32 + grad_acc_row(v, hh)) * N + i] = acc[v];
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

#undef GRAD_LANE_IDS

}  // namespace sfa
