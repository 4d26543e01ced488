// Kernels of sfa_model_block_grad / sfa_bn_unfold_grad (gfx950): the gradients of one BasicBlock
// (models/fpn_resnet.py:42-71) with its BatchNorms folded, block_plan.h has the shapes.
//
// One GEMM family on grad_tile.h's 64 x 64 tile (v_mfma_f32_32x32x2_f32, 2 x 2 waves, K walked in steps of kGradStep
// through two k-major LDS tiles); the next step's global loads are issued into registers before the step's 8 MFMAs.
//   block_dgrad_kernel   a 3x3 / pad 1 / stride s data gradient as an implicit GEMM: rows = 64 flat pixels of the
//                        convolution's INPUT map, columns = 64 input channels, K = (tap, o) = 9 cout, plus a second
//                        segment of cout for the 1x1 stride-s downsample read as the centre tap; all of K inside one
//                        workgroup, in that order.  The A operand is gathered: input pixel (iy, ix) and tap (ky, kx)
//                        meet output pixel ((iy + 1 - ky) / s, (ix + 1 - kx) / s) when both divide and lie inside
//                        the map, else zero.  A ReLU mask on the operand (dZ = y > 0 ? gy : 0) is applied as it is
//                        loaded; the epilogue adds the identity skip's masked gradient and / or applies the mask of
//                        the map the result belongs to (dA = a > 0 ? . : 0).  Every element stored once by one lane.
//   block_wgrad_kernel   rows = cout, columns = 64 input channels of one tap, K = the output pixels of one split-K
//                        chunk: dZ / dA rows as they lie (masked on load), the x rows gathered through the tap;
//                        float32 partial tile per chunk (grad_common.hip's fold adds the chunks into torch's
//                        (cout, cin, kh, kw) layout and its bias pair computes db, masked on load)
//   bn_unfold_kernel     folded gradients -> the convolution's and the BatchNorm's, float64 from float32 operands
//
// No atomics; every sum has a fixed order, so runs are bit-identical.
#pragma once

#include "block_plan.h"  // BkDgrad, BkWgrad
#include "grad_tile.h"

namespace sfa {

// out[p][i] = sum over (tap, o) of g0[src(p, tap)][o] W0[o][tap cin + i] + sum over o of g1[src(p, centre)][o] W1[o][i]
// grid (grad_tiles(npix), cin / 64), block (256)
__global__ void __launch_bounds__(256) block_dgrad_kernel(BkDgrad t, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float sA[kGradLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kGradLdsWords];
  GRAD_LANE_IDS;
  const GradRange pt = grad_tile_at((int)blockIdx.x, t.npix);
  const int i0 = (int)blockIdx.y * kGradTile;
  const int spt = t.cout / kGradStep;                 // steps of one tap
  const int steps = (t.g1 ? 10 : 9) * spt;
  // this thread's A row: pixel pt.first + tid / 4 of the input map
  const int am = tid >> 2, aq = (tid & 3) * 4;
  const bool a_live = am < pt.count;
  int ab = 0, aiy = 0, aix = 0;
  if (a_live) {
    const int p = pt.first + am;
    aix = p % t.w;
    const int q = p / t.w;
    aiy = q % t.h;
    ab = q / t.h;
  }
  const int bk = tid >> 4, bq = (tid & 15) * 4;     // this thread's B k row and column quad
  auto load_a = [&](int step) -> grad_f32x4 {
    const int tap = step / spt, o0 = (step - tap * spt) * kGradStep;
    const bool seg1 = tap == 9;
    const int ky = seg1 ? 1 : tap / 3, kx = seg1 ? 1 : tap - 3 * (tap / 3);
    if (!a_live) return grad_zero4();
    const int oy = block_tap_source(aiy, ky, t.s, t.oh), ox = block_tap_source(aix, kx, t.s, t.ow);
    if (oy < 0 || ox < 0) return grad_zero4();
    const size_t at = ((size_t)(ab * t.oh + oy) * t.ow + ox) * t.cout + o0 + aq;
    return seg1 ? grad_load_masked(t.g1, t.m1, at) : grad_load_masked(t.g0, t.m0, at);
  };
  auto load_b = [&](int step) -> grad_f32x4 {
    const int tap = step / spt, o = (step - tap * spt) * kGradStep + bk;
    const float* src = tap == 9 ? t.W1 + (size_t)o * t.ldw1 + i0 + bq : t.W0 + (size_t)o * t.ldw0 + tap * t.cin + i0 + bq;
    return *reinterpret_cast<const grad_f32x4*>(src);
  };
  grad_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  grad_f32x4 ra = load_a(0), rb = load_b(0);
  for (int step = 0; step < steps; ++step) {
    __syncthreads();  // the previous step's fragment reads are done
    grad_store_kc(sA, ra, tid);
    grad_store_mc(sB, rb, tid);
    __syncthreads();
    if (step + 1 < steps) {
      ra = load_a(step + 1);
      rb = load_b(step + 1);
    }
    grad_mma(sA, sB, wm, wn, r, hh, acc);
  }
  const int i = i0 + wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = wm * 32 + grad_acc_row(v, hh);
    if (q < pt.count) {
      const size_t at = (size_t)(pt.first + q) * t.cin + i;
      float val = acc[v];
      if (t.eg) val = val + ((!t.em || t.em[at] > 0.f) ? t.eg[at] : 0.f);
      if (t.om) val = t.om[at] > 0.f ? val : 0.f;
      out[at] = val;
    }
  }
}

// part[chunk][o][(tap - tap0) cin + c] = sum over the chunk's output pixels p of g[p][o] x[src(p, tap)][c]
// grid (chunks, ntaps cin / 64, M / 64), block (256)
__global__ void __launch_bounds__(256) block_wgrad_kernel(BkWgrad t, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sA[kGradLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kGradLdsWords];
  GRAD_LANE_IDS;
  const GradRange ck = grad_chunk_at((int)blockIdx.x, t.npix, t.Kc);
  const int ctiles = t.cin / kGradTile;
  const int tapi = (int)blockIdx.y / ctiles, c0 = ((int)blockIdx.y - tapi * ctiles) * kGradTile;
  const int tap = t.tap0 + tapi, ky = tap / 3, kx = tap - 3 * ky;
  const int o0 = (int)blockIdx.z * kGradTile, N = t.ntaps * t.cin;
  const int kk = tid >> 4, q4 = (tid & 15) * 4;  // this thread's k row (pixel of the step) and column quad
  auto load_g = [&](int k) -> grad_f32x4 {
    if (k + kk >= ck.count) return grad_zero4();  // a short last step pairs with zero rows
    return grad_load_masked(t.g, t.gm, (size_t)(ck.first + k + kk) * t.M + o0 + q4);
  };
  auto load_x = [&](int k) -> grad_f32x4 {
    if (k + kk >= ck.count) return grad_zero4();
    const int p = ck.first + k + kk;
    const int ox = p % t.ow, q = p / t.ow;
    const int oy = q % t.oh, b = q / t.oh;
    const int iy = oy * t.s - 1 + ky, ix = ox * t.s - 1 + kx;
    if ((unsigned)iy >= (unsigned)t.h || (unsigned)ix >= (unsigned)t.w) return grad_zero4();
    return *reinterpret_cast<const grad_f32x4*>(t.x + ((size_t)(b * t.h + iy) * t.w + ix) * t.cin + c0 + q4);
  };
  grad_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  grad_f32x4 ra = load_g(0), rb = load_x(0);
  for (int k = 0; k < ck.count; k += kGradStep) {
    __syncthreads();
    grad_store_mc(sA, ra, tid);
    grad_store_mc(sB, rb, tid);
    __syncthreads();
    if (k + kGradStep < ck.count) {
      ra = load_g(k + kGradStep);
      rb = load_x(k + kGradStep);
    }
    grad_mma(sA, sB, wm, wn, r, hh, acc);
  }
  float* P = part + (size_t)blockIdx.x * t.M * N;
  const int col = tapi * t.cin + c0 + wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) P[(size_t)(o0 + wm * 32 + grad_acc_row(v, hh)) * N + col] = acc[v];
}

// Row o of a folded convolution W' = s W, b' = beta - mean s, s = gamma / sqrt(var + eps):
//   dW[o][k] = s dW'[o][k],  dbeta[o] = db'[o],  dgamma[o] = (sum_k W[o][k] dW'[o][k] - mean[o] db'[o]) / sqrt(var[o] + eps)
// in float64 from the float32 operands, rounded once.  The sum: per thread over k = t, t + 256, .. in that order, then
// the 256 threads by a fixed tree.  Outputs that are null are skipped.
// grid (Cout), block (256)
__global__ void __launch_bounds__(256) bn_unfold_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                        const float* __restrict__ mean, const float* __restrict__ var,
                                                        double eps, const float* __restrict__ dWf,
                                                        const float* __restrict__ dbf, int K, float* __restrict__ dW,
                                                        float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double red[256];
  const int o = blockIdx.x, tid = threadIdx.x;
  const double sd = sqrt((double)var[o] + eps);
  const double sc = (double)gamma[o] / sd;
  double s = 0.0;
  if (dWf)
    for (int k = tid; k < K; k += 256) {
      const double g = (double)dWf[(size_t)o * K + k];
      if (dW) dW[(size_t)o * K + k] = (float)(sc * g);
      if (dgamma) s += (double)W[(size_t)o * K + k] * g;
    }
  if (!dgamma) {
    if (tid == 0 && dbeta) dbeta[o] = dbf[o];
    return;
  }
  red[tid] = s;
  __syncthreads();
  for (int n = 128; n >= 1; n >>= 1) {
    if (tid < n) red[tid] += red[tid + n];
    __syncthreads();
  }
  if (tid == 0) {
    dgamma[o] = (float)((red[0] - (double)mean[o] * (double)dbf[o]) / sd);
    if (dbeta) dbeta[o] = dbf[o];
  }
}

#undef GRAD_LANE_IDS

}  // namespace sfa
