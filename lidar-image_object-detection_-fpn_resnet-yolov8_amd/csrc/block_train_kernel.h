// Kernels of sfa_block_train_forward / sfa_block_train_grad (gfx950): one BasicBlock (models/fpn_resnet.py:42-71)
// with its BatchNorms in training mode, block_train_plan.h has the shapes.  The data and weight gradients of the
// convolutions are block_kernel.h's, launched through block_host.h.
//   block_conv_fwd_kernel    z = conv(x; W), no bias, no ReLU: a forward implicit GEMM on grad_tile.h's 64 x 64 tile
//                            (v_mfma_f32_32x32x2_f32): rows = 64 flat output pixels, columns = 64 output channels,
//                            K = (tap, c) in that order, all of it inside one workgroup.  The A operand is gathered:
//                            output pixel (oy, ox) and tap (ky, kx) read input pixel (oy s - 1 + ky, ox s - 1 + kx),
//                            zero outside the map (every row and column is tested, so odd sizes work at stride 2);
//                            the B operand is the k-major copy [tap cin + c][o] of W.  3x3 at stride 1 or 2, and the
//                            1x1 stride-2 downsample as the centre tap alone.
//   block_w_relayout_kernel  torch's (Cout, Cin, kh, kw) -> [tap cin + c][o] and / or [o][tap cin + c]
//   bn_stats_kernel + fold   per (pixel block, channel) float64 sums of z and z^2 in pixel order, then over the
//                            blocks in block order: mean = S1 / n, var = max(S2 / n - mean^2, 0) (biased), each
//                            rounded once to float32; the fold also leaves the float32 pair
//                            s = gamma / sqrt(var + eps), t = beta - mean s, computed in float64 from the ROUNDED
//                            mean and var (what a later call recomputes from the statistics array) and rounded once
//   bn_apply_kernel          v = fmaf(s, z, t) [+ x  |  + fmaf(sd, zd, td)], out = max(v, 0): float32, one FMA per
//                            BatchNorm, one addition for the skip
//   bn_bwd_reduce_kernel + fold   A = sum dY, Bq = sum dY (z - mean) in float64 (dY masked as it is loaded), the
//                            fold writes dbeta = A, dgamma = invstd Bq (rounded once) and keeps (A, Bq) in float64
//   bn_bwd_apply_kernel      dZ = gamma invstd (dY - A / n - (z - mean) invstd^2 Bq / n) in float64, rounded once
// No atomics; every sum has a fixed order, so runs are bit-identical.
#pragma once

#include "block_train_plan.h"
#include "grad_tile.h"

namespace sfa {

// One forward convolution: x (B, h, w, cin) through taps tap0 .. tap0 + ntaps - 1 of the 3x3 / pad 1 / stride s
// window, Wk [(tap - tap0) cin + c][cout]; z (B, oh, ow, cout), npix = B oh ow.
struct BkConvFwd {
  const float *x, *Wk;
  int h, w, oh, ow, s, cin, cout, tap0, ntaps, npix;
};

// z[p][o] = sum over (tap, c) of x[in(p, tap)][c] Wk[(tap - tap0) cin + c][o]
// grid (grad_tiles(npix), cout / 64), block (256)
__global__ void __launch_bounds__(256) block_conv_fwd_kernel(BkConvFwd t, float* __restrict__ z) {
  __shared__ __attribute__((aligned(16))) float sA[kGradLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kGradLdsWords];
  GRAD_LANE_IDS;
  const GradRange pt = grad_tile_at((int)blockIdx.x, t.npix);
  const int o0 = (int)blockIdx.y * kGradTile;
  const int spt = t.cin / kGradStep;  // steps of one tap
  const int steps = t.ntaps * spt;
  // this thread's A row: output pixel pt.first + tid / 4
  const int am = tid >> 2, aq = (tid & 3) * 4;
  const bool a_live = am < pt.count;
  int ab = 0, aoy = 0, aox = 0;
  if (a_live) {
    const int p = pt.first + am;
    aox = p % t.ow;
    const int q = p / t.ow;
    aoy = q % t.oh;
    ab = q / t.oh;
  }
  const int bk = tid >> 4, bq = (tid & 15) * 4;  // this thread's B k row and column quad
  auto load_a = [&](int step) -> grad_f32x4 {
    const int tapi = step / spt, c0 = (step - tapi * spt) * kGradStep;
    const int tap = t.tap0 + tapi, ky = tap / 3, kx = tap - 3 * ky;
    if (!a_live) return grad_zero4();
    const int iy = block_train_tap_input(aoy, ky, t.s, t.h), ix = block_train_tap_input(aox, kx, t.s, t.w);
    if (iy < 0 || ix < 0) return grad_zero4();
    return *reinterpret_cast<const grad_f32x4*>(t.x + ((size_t)(ab * t.h + iy) * t.w + ix) * t.cin + c0 + aq);
  };
  auto load_b = [&](int step) -> grad_f32x4 {  // k row step * kGradStep + bk = (tap - tap0) cin + c
    return *reinterpret_cast<const grad_f32x4*>(t.Wk + (size_t)(step * kGradStep + bk) * t.cout + o0 + bq);
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
  const int o = o0 + wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = wm * 32 + grad_acc_row(v, hh);
    if (q < pt.count) z[(size_t)(pt.first + q) * t.cout + o] = acc[v];
  }
}

// W (cout, cin, taps) as torch lays it -> Wk [tap cin + c][o] and Wt [o][tap cin + c], each skipped when null.
// grid (ceil(cout taps cin / 256)), block (256): thread e = (o, tap, c)
__global__ void __launch_bounds__(256) block_w_relayout_kernel(const float* __restrict__ W, int cout, int cin, int taps,
                                                               float* __restrict__ Wk, float* __restrict__ Wt) {
  const int K = taps * cin;
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= cout * K) return;
  const int o = e / K, k = e - o * K;
  const int tap = k / cin, c = k - tap * cin;
  const float v = W[((size_t)o * cin + c) * taps + tap];
  if (Wt) Wt[e] = v;
  if (Wk) Wk[(size_t)k * cout + o] = v;
}

// part[block][o] = (sum z, sum z^2) over the block's run of pixels, float64, pixel order.
// grid (blocks, ceil(cout / 256)), block (256): thread o
__global__ void __launch_bounds__(256) bn_stats_kernel(const float* __restrict__ z, double* __restrict__ part, int npix,
                                                       int pixels, int cout) {
  const GradRange run = grad_chunk_at((int)blockIdx.x, npix, pixels);
  const int o = (int)blockIdx.y * 256 + (int)threadIdx.x;
  if (o >= cout) return;
  double s1 = 0.0, s2 = 0.0;
  for (int p = run.first; p < run.first + run.count; ++p) {
    const double v = (double)z[(size_t)p * cout + o];
    s1 += v;
    s2 += v * v;
  }
  double* P = part + ((size_t)blockIdx.x * cout + o) * 2;
  P[0] = s1, P[1] = s2;
}

// The float32 pair of one channel from the float32 statistics: s = gamma / sqrt(var + eps), t = beta - mean s.
__device__ __forceinline__ void bn_train_coef(float gamma, float beta, float mean, float var, double eps, float* s,
                                              float* t) {
  const double sc = (double)gamma / sqrt((double)var + eps);
  *s = (float)sc;
  *t = (float)((double)beta - (double)mean * sc);
}

// stats [2][cout] = (mean, biased var), coef [2][cout] = (s, t).  grid (ceil(cout / 256)), block (256)
__global__ void __launch_bounds__(256) bn_stats_fold_kernel(const double* __restrict__ part, int blocks, int cout, int n,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, double eps,
                                                            float* __restrict__ stats, float* __restrict__ coef) {
  const int o = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (o >= cout) return;
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < blocks; ++b) {
    s1 += part[((size_t)b * cout + o) * 2];
    s2 += part[((size_t)b * cout + o) * 2 + 1];
  }
  const double mean = s1 / (double)n;
  double var = s2 / (double)n - mean * mean;
  if (!(var > 0.0)) var = 0.0;
  const float mf = (float)mean, vf = (float)var;
  stats[o] = mf;
  stats[cout + o] = vf;
  bn_train_coef(gamma[o], beta[o], mf, vf, eps, coef + o, coef + cout + o);
}

// out = max(fmaf(s, z, t) + skip, 0); skip: x (identity, zd null), fmaf(sd, zd, td) (cd not null), or nothing (both
// null).  coef [2][cout].  grid (ceil(npix cout / 4 / 256)), block (256): one float4 per thread
__global__ void __launch_bounds__(256) bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ c,
                                                       const float* __restrict__ x, const float* __restrict__ zd,
                                                       const float* __restrict__ cd, float* __restrict__ out, int quads,
                                                       int cout) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= quads) return;
  const size_t at = (size_t)e * 4;
  const int o = (int)(at % (size_t)cout);
  const grad_f32x4 zv = *reinterpret_cast<const grad_f32x4*>(z + at);
  const grad_f32x4 sv = *reinterpret_cast<const grad_f32x4*>(c + o);
  const grad_f32x4 tv = *reinterpret_cast<const grad_f32x4*>(c + cout + o);
  grad_f32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = __builtin_fmaf(sv[i], zv[i], tv[i]);
  if (zd) {
    const grad_f32x4 dv = *reinterpret_cast<const grad_f32x4*>(zd + at);
    const grad_f32x4 sd = *reinterpret_cast<const grad_f32x4*>(cd + o);
    const grad_f32x4 td = *reinterpret_cast<const grad_f32x4*>(cd + cout + o);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] + __builtin_fmaf(sd[i], dv[i], td[i]);
  } else if (x) {
    const grad_f32x4 xv = *reinterpret_cast<const grad_f32x4*>(x + at);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] + xv[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.f ? v[i] : 0.f;
  *reinterpret_cast<grad_f32x4*>(out + at) = v;
}

// part[block][o] = (sum dY, sum dY (z - mean)) over the block's run of pixels, float64, pixel order; dY = g where
// gm > 0 (g itself when gm is null).  stats [2][cout].  grid (blocks, ceil(cout / 256)), block (256): thread o
__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(const float* __restrict__ g, const float* __restrict__ gm,
                                                            const float* __restrict__ z,
                                                            const float* __restrict__ stats, double* __restrict__ part,
                                                            int npix, int pixels, int cout) {
  const GradRange run = grad_chunk_at((int)blockIdx.x, npix, pixels);
  const int o = (int)blockIdx.y * 256 + (int)threadIdx.x;
  if (o >= cout) return;
  const double mean = (double)stats[o];
  double a = 0.0, b = 0.0;
  for (int p = run.first; p < run.first + run.count; ++p) {
    const size_t at = (size_t)p * cout + o;
    const double dy = (double)((!gm || gm[at] > 0.f) ? g[at] : 0.f);
    a += dy;
    b += dy * ((double)z[at] - mean);
  }
  double* P = part + ((size_t)blockIdx.x * cout + o) * 2;
  P[0] = a, P[1] = b;
}

// sums [cout][2] = (A, Bq) over the blocks in block order; dbeta = A and dgamma = Bq / sqrt(var + eps), each skipped
// when null.  grid (ceil(cout / 256)), block (256)
__global__ void __launch_bounds__(256) bn_bwd_fold_kernel(const double* __restrict__ part, int blocks, int cout,
                                                          const float* __restrict__ stats, double eps,
                                                          double* __restrict__ sums, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta) {
  const int o = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (o >= cout) return;
  double a = 0.0, b = 0.0;
  for (int k = 0; k < blocks; ++k) {
    a += part[((size_t)k * cout + o) * 2];
    b += part[((size_t)k * cout + o) * 2 + 1];
  }
  sums[(size_t)o * 2] = a;
  sums[(size_t)o * 2 + 1] = b;
  if (dbeta) dbeta[o] = (float)a;
  if (dgamma) dgamma[o] = (float)(b / sqrt((double)stats[cout + o] + eps));
}

// dZ = gamma invstd (dY - A / n - (z - mean) invstd^2 Bq / n), float64 per element, rounded once.
// grid (ceil(npix cout / 256)), block (256): one element per thread
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ gm,
                                                           const float* __restrict__ z, const float* __restrict__ stats,
                                                           const float* __restrict__ gamma,
                                                           const double* __restrict__ sums, double eps, int n, int total,
                                                           int cout, float* __restrict__ dz) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= total) return;
  const int o = e % cout;
  const double mean = (double)stats[o];
  const double invstd = 1.0 / sqrt((double)stats[cout + o] + eps);
  const double dy = (double)((!gm || gm[e] > 0.f) ? g[e] : 0.f);
  const double a = sums[(size_t)o * 2] / (double)n;
  const double b = sums[(size_t)o * 2 + 1] / (double)n;
  const double xc = (double)z[e] - mean;
  dz[e] = (float)((double)gamma[o] * invstd * (dy - a - xc * (invstd * invstd) * b));
}

#undef GRAD_LANE_IDS

}  // namespace sfa
