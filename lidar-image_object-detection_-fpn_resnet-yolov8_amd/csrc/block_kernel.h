// Kernels of sfa_model_block_grad / sfa_bn_unfold_grad (gfx950): the gradients of one BasicBlock
// (models/fpn_resnet.py:42-71) with its BatchNorms folded, block_plan.h has the shapes.
//
// One GEMM family on v_mfma_f32_32x32x2_f32 as neck_kernel.h's: a workgroup of 2 x 2 waves owns a 64 x 64 tile with
// one 16-register accumulator per wave, K walked in steps of kBkStep through two LDS tiles held k-major ([k][64],
// rows kBkLd words apart); the next step's global loads are issued into registers before the step's 8 MFMAs.
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
//                        float32 partial tile per chunk
//   block_wgrad_fold_kernel   per dW element: the chunks added in chunk order in float64, rounded once, written in
//                        torch's (cout, cin, kh, kw) layout
//   block_bias_kernel, block_bias_fold_kernel   db: float64 sums over runs of pixels in pixel order (masked on
//                        load), then over the runs in run order, rounded once
//   bn_unfold_kernel     folded gradients -> the convolution's and the BatchNorm's, float64 from float32 operands
//
// No atomics; every sum has a fixed order, so runs are bit-identical.
#pragma once

#include "block_plan.h"
#include "block_tile.h"
#include "common.h"

namespace sfa {

// The maps of one data gradient.  g0 (B, oh, ow, cout), masked by m0 when it is not null, meets W0 [o][tap cin + c]
// (row stride ldw0) through the nine taps; g1 / m1 / W1 [o][c] (row stride ldw1), when g1 is not null, through the
// centre tap alone.  eg / em: the masked map the epilogue adds (same shape as out), or null.  om: the map whose sign
// masks the result, or null.
struct BkDgrad {
  const float *g0, *m0, *W0, *g1, *m1, *W1, *eg, *em, *om;
  int ldw0, ldw1;
  int h, w, oh, ow, s, cin, cout, npix;  // out is (B, h, w, cin), npix = B h w
};

// out[p][i] = sum over (tap, o) of g0[src(p, tap)][o] W0[o][tap cin + i] + sum over o of g1[src(p, centre)][o] W1[o][i]
// grid (block_tiles(npix), cin / 64), block (256)
__global__ void __launch_bounds__(256) block_dgrad_kernel(BkDgrad t, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float sA[kBkLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kBkLdsWords];
  BK_LANE_IDS;
  const BlockRange pt = block_tile_at((int)blockIdx.x, t.npix);
  const int i0 = (int)blockIdx.y * kBkTile;
  const int spt = t.cout / kBkStep;                 // steps of one tap
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
  auto load_a = [&](int step) -> bk_f32x4 {
    const int tap = step / spt, o0 = (step - tap * spt) * kBkStep;
    const bool seg1 = tap == 9;
    const int ky = seg1 ? 1 : tap / 3, kx = seg1 ? 1 : tap - 3 * (tap / 3);
    if (!a_live) return bk_zero4();
    const int oy = block_tap_source(aiy, ky, t.s, t.oh), ox = block_tap_source(aix, kx, t.s, t.ow);
    if (oy < 0 || ox < 0) return bk_zero4();
    const size_t at = ((size_t)(ab * t.oh + oy) * t.ow + ox) * t.cout + o0 + aq;
    return seg1 ? bk_load_masked(t.g1, t.m1, at) : bk_load_masked(t.g0, t.m0, at);
  };
  auto load_b = [&](int step) -> bk_f32x4 {
    const int tap = step / spt, o = (step - tap * spt) * kBkStep + bk;
    const float* src = tap == 9 ? t.W1 + (size_t)o * t.ldw1 + i0 + bq : t.W0 + (size_t)o * t.ldw0 + tap * t.cin + i0 + bq;
    return *reinterpret_cast<const bk_f32x4*>(src);
  };
  bk_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  bk_f32x4 ra = load_a(0), rb = load_b(0);
  for (int step = 0; step < steps; ++step) {
    __syncthreads();  // the previous step's fragment reads are done
    bk_store_kc(sA, ra, tid);
    bk_store_mc(sB, rb, tid);
    __syncthreads();
    if (step + 1 < steps) {
      ra = load_a(step + 1);
      rb = load_b(step + 1);
    }
    bk_mma(sA, sB, wm, wn, r, hh, acc);
  }
  const int i = i0 + wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = wm * 32 + bk_acc_row(v, hh);
    if (q < pt.count) {
      const size_t at = (size_t)(pt.first + q) * t.cin + i;
      float val = acc[v];
      if (t.eg) val = val + ((!t.em || t.em[at] > 0.f) ? t.eg[at] : 0.f);
      if (t.om) val = t.om[at] > 0.f ? val : 0.f;
      out[at] = val;
    }
  }
}

// One weight gradient.  g (B, oh, ow, M) masked by gm when it is not null; x (B, h, w, cin) read through taps
// tap0 .. tap0 + ntaps - 1 of the 3x3 / pad 1 / stride s window.
struct BkWgrad {
  const float *g, *gm, *x;
  int h, w, oh, ow, s, cin, M, tap0, ntaps, npix, Kc;  // npix = B oh ow
};

// part[chunk][o][(tap - tap0) cin + c] = sum over the chunk's output pixels p of g[p][o] x[src(p, tap)][c]
// grid (chunks, ntaps cin / 64, M / 64), block (256)
__global__ void __launch_bounds__(256) block_wgrad_kernel(BkWgrad t, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sA[kBkLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kBkLdsWords];
  BK_LANE_IDS;
  const BlockRange ck = block_chunk_at((int)blockIdx.x, t.npix, t.Kc);
  const int ctiles = t.cin / kBkTile;
  const int tapi = (int)blockIdx.y / ctiles, c0 = ((int)blockIdx.y - tapi * ctiles) * kBkTile;
  const int tap = t.tap0 + tapi, ky = tap / 3, kx = tap - 3 * ky;
  const int o0 = (int)blockIdx.z * kBkTile, N = t.ntaps * t.cin;
  const int kk = tid >> 4, q4 = (tid & 15) * 4;  // this thread's k row (pixel of the step) and column quad
  auto load_g = [&](int k) -> bk_f32x4 {
    if (k + kk >= ck.count) return bk_zero4();  // a short last step pairs with zero rows
    return bk_load_masked(t.g, t.gm, (size_t)(ck.first + k + kk) * t.M + o0 + q4);
  };
  auto load_x = [&](int k) -> bk_f32x4 {
    if (k + kk >= ck.count) return bk_zero4();
    const int p = ck.first + k + kk;
    const int ox = p % t.ow, q = p / t.ow;
    const int oy = q % t.oh, b = q / t.oh;
    const int iy = oy * t.s - 1 + ky, ix = ox * t.s - 1 + kx;
    if ((unsigned)iy >= (unsigned)t.h || (unsigned)ix >= (unsigned)t.w) return bk_zero4();
    return *reinterpret_cast<const bk_f32x4*>(t.x + ((size_t)(b * t.h + iy) * t.w + ix) * t.cin + c0 + q4);
  };
  bk_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  bk_f32x4 ra = load_g(0), rb = load_x(0);
  for (int k = 0; k < ck.count; k += kBkStep) {
    __syncthreads();
    bk_store_mc(sA, ra, tid);
    bk_store_mc(sB, rb, tid);
    __syncthreads();
    if (k + kBkStep < ck.count) {
      ra = load_g(k + kBkStep);
      rb = load_x(k + kBkStep);
    }
    bk_mma(sA, sB, wm, wn, r, hh, acc);
  }
  float* P = part + (size_t)blockIdx.x * t.M * N;
  const int col = tapi * t.cin + c0 + wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) P[(size_t)(o0 + wm * 32 + bk_acc_row(v, hh)) * N + col] = acc[v];
}

// dW[o][c][tap] ((M, cin, ntaps) contiguous: torch's (M, cin, 3, 3) or (M, cin, 1, 1)) = the chunks of
// part[chunk][o][tap cin + c] added in chunk order.
// grid (ceil(M ntaps cin / 256)), block (256)
__global__ void __launch_bounds__(256) block_wgrad_fold_kernel(const float* __restrict__ part, int chunks, int M, int cin,
                                                               int ntaps, float* __restrict__ dW) {
  const int N = ntaps * cin;
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= M * N) return;
  const int o = e / N, rem = e - o * N;
  const int tap = rem / cin, c = rem - tap * cin;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += (double)part[(size_t)k * M * N + e];
  dW[((size_t)o * cin + c) * ntaps + tap] = (float)s;
}

// grid (blocks, ceil(cout / 256)), block (256): thread o adds g[p][o] (masked by gm) over the block's run of pixels.
// part: [block][cout].
__global__ void __launch_bounds__(256) block_bias_kernel(const float* __restrict__ g, const float* __restrict__ gm,
                                                         double* __restrict__ part, int npix, int pixels, int cout) {
  const BlockRange run = block_chunk_at((int)blockIdx.x, npix, pixels);
  const int o = (int)blockIdx.y * 256 + (int)threadIdx.x;
  if (o >= cout) return;
  double s = 0.0;
  for (int p = run.first; p < run.first + run.count; ++p) {
    const size_t at = (size_t)p * cout + o;
    const float v = g[at];
    s += (double)((!gm || gm[at] > 0.f) ? v : 0.f);
  }
  part[(size_t)blockIdx.x * cout + o] = s;
}

// grid (ceil(cout / 256)), block (256)
__global__ void __launch_bounds__(256) block_bias_fold_kernel(const double* __restrict__ part, int blocks, int cout,
                                                              float* __restrict__ db) {
  const int o = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (o >= cout) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += part[(size_t)b * cout + o];
  db[o] = (float)s;
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

#undef BK_LANE_IDS

}  // namespace sfa
