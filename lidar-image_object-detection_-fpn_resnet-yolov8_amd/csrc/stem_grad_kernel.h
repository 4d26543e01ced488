// Kernels of sfa_model_stem_grad (gfx950): the gradients of the stem (models/fpn_resnet.py:179-182: conv1 7x7 / 2 /
// pad 3 with bn1 folded, ReLU, MaxPool2d(3, 2, 1)); stem_grad_plan.h has the shapes and the source functions.
//   stem_pool_adjoint_kernel   dA = a > 0 ? (pool adjoint of gp) : 0 as a gather over the pixels of a: a pixel looks
//                        at the (at most 4) windows that hold it and takes a window's gp exactly when it is that
//                        window's first maximum in row-major scan order (strict > before it, >= after it: torch's
//                        rule; padding never wins because it is never read).  Every element stored once by one lane.
//   stem_wgrad_kernel    dW' on v_mfma_f32_32x32x2_f32 with grad_tile.h's 64 x 64 tile: rows = the 64 output
//                        channels, columns = 64 of the 147 (c, ky, kx) entries padded to 192, K = the conv output
//                        pixels of one split-K chunk.  dA rows as they lie; the x operand gathered from the NCHW
//                        image, every row and column tested against H and W.  float32 partial tile per chunk
//                        [chunk][64][147]; grad_wgrad_fold_kernel adds the chunks (grad_common.hip).
//   stem_dgrad_kernel    dx as a vector gather: one image pixel per thread, the taps whose parity matches
//                        (ky = iy + 3 mod 2, likewise kx; stem_tap_source) in (ky, kx) order, the 64 channels in
//                        channel order, three float64 accumulators (one per input plane) from exact float32
//                        products, rounded once.  W' [tap][o] as float4 (c0, c1, c2, 0) in LDS: the handle's
//                        packed row order.
// db' is grad_bias_kernel on dA (grad_common.hip).  No atomics; every sum has a fixed order, so runs are bit-identical.
#pragma once

#include "grad_tile.h"
#include "stem_grad_plan.h"

namespace sfa {

// grid (ceil(npix 16 / 256)), block (256): thread = (pixel of a, channel quad)
__global__ void __launch_bounds__(256) stem_pool_adjoint_kernel(const float* __restrict__ a, const float* __restrict__ gp,
                                                                float* __restrict__ dA, int oh, int ow, int ph, int pw,
                                                                int npix) {
  const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const int p = idx >> 4, q = (idx & 15) * 4;
  if (p >= npix) return;
  const int x = p % ow, t = p / ow;
  const int y = t % oh, b = t / oh;
  const grad_f32x4 me = *reinterpret_cast<const grad_f32x4*>(a + (size_t)p * kSgC + q);
  grad_f32x4 out = grad_zero4();
  if (me.x > 0.f || me.y > 0.f || me.z > 0.f || me.w > 0.f) {
    const int wy0 = stem_pool_first_window(y), ny = stem_pool_windows(y, ph);
    const int wx0 = stem_pool_first_window(x), nx = stem_pool_windows(x, pw);
    for (int jy = 0; jy < ny; ++jy)
      for (int jx = 0; jx < nx; ++jx) {
        const int wy = wy0 + jy, wx = wx0 + jx;
        int w0 = 1, w1 = 1, w2 = 1, w3 = 1;  // still the window's first maximum, per channel
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          const int iy = 2 * wy - 1 + dy;
          if ((unsigned)iy >= (unsigned)oh) continue;
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * wx - 1 + dx;
            if ((unsigned)ix >= (unsigned)ow || (iy == y && ix == x)) continue;
            const grad_f32x4 v =
                *reinterpret_cast<const grad_f32x4*>(a + ((size_t)(b * oh + iy) * ow + ix) * kSgC + q);
            // scanned before this pixel: it must be strictly smaller; after it: not larger
            const bool before = iy < y || (iy == y && ix < x);
            w0 &= (int)(before ? v.x < me.x : v.x <= me.x);
            w1 &= (int)(before ? v.y < me.y : v.y <= me.y);
            w2 &= (int)(before ? v.z < me.z : v.z <= me.z);
            w3 &= (int)(before ? v.w < me.w : v.w <= me.w);
          }
        }
        const grad_f32x4 g = *reinterpret_cast<const grad_f32x4*>(gp + ((size_t)(b * ph + wy) * pw + wx) * kSgC + q);
        out.x = out.x + (w0 ? g.x : 0.f), out.y = out.y + (w1 ? g.y : 0.f);
        out.z = out.z + (w2 ? g.z : 0.f), out.w = out.w + (w3 ? g.w : 0.f);
      }
    out = grad_masked(out, me);
  }
  *reinterpret_cast<grad_f32x4*>(dA + (size_t)p * kSgC + q) = out;
}

// part[chunk][o][j] = sum over the chunk's conv output pixels p of dA[p][o] x[b][c][2 oy - 3 + ky][2 ox - 3 + kx],
// j = (c, ky, kx) < 147.  grid (chunks, kSgColTiles), block (256)
__global__ void __launch_bounds__(256) stem_wgrad_kernel(const float* __restrict__ dA, const float* __restrict__ x,
                                                         float* __restrict__ part, int H, int W, int oh, int ow, int npix,
                                                         int Kc) {
  __shared__ __attribute__((aligned(16))) float sA[kGradLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kGradLdsWords];
  GRAD_LANE_IDS;
  const GradRange ck = grad_chunk_at((int)blockIdx.x, npix, Kc);
  const int j0 = (int)blockIdx.y * kGradTile;
  const int kk = tid >> 4, q4 = (tid & 15) * 4;  // this thread's k row (pixel of the step) and column quad
  // this thread's four columns: plane offset and tap of each (a column past 146 reads nothing)
  int cpl[4], cky[4], ckx[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = j0 + q4 + e;
    int c = 0, ky = 0, kx = 0;
    if (j < kSgK) stem_column(j, &c, &ky, &kx);
    cpl[e] = j < kSgK ? c : -1, cky[e] = ky, ckx[e] = kx;
  }
  auto load_g = [&](int k) -> grad_f32x4 {
    if (k + kk >= ck.count) return grad_zero4();  // a short last step pairs with zero rows
    return *reinterpret_cast<const grad_f32x4*>(dA + (size_t)(ck.first + k + kk) * kSgC + q4);
  };
  auto load_x = [&](int k) -> grad_f32x4 {
    grad_f32x4 v = grad_zero4();
    if (k + kk >= ck.count) return v;
    const int p = ck.first + k + kk;
    const int ox = p % ow, q = p / ow;
    const int oy = q % oh, b = q / oh;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int iy = 2 * oy - 3 + cky[e], ix = 2 * ox - 3 + ckx[e];
      if (cpl[e] >= 0 && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
        v[e] = x[((size_t)(b * 3 + cpl[e]) * H + iy) * W + ix];
    }
    return v;
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
  float* P = part + (size_t)blockIdx.x * kSgC * kSgK;
  const int col = j0 + wn * 32 + r;
  if (col < kSgK) {
#pragma unroll
    for (int v = 0; v < 16; ++v) P[(size_t)(wm * 32 + grad_acc_row(v, hh)) * kSgK + col] = acc[v];
  }
}

// dx[b][c][iy][ix] = sum over (ky, kx) of matching parity, o of dA[b][oy][ox][o] W'[o][c][ky][kx], oy = stem_tap_source(iy,
// ky, oh), ox likewise.  Wp: the handle's packed rows [o][(ky 7 + kx) 4 + c] of ldw words.
// grid (min(ceil(npix / 256), kSgDgradMaxBlocks)), block (256): passes of 256 consecutive image pixels.
__global__ void __launch_bounds__(256) stem_dgrad_kernel(const float* __restrict__ dA, const float* __restrict__ Wp, int ldw,
                                                         float* __restrict__ dx, int H, int W, int oh, int ow, int npix) {
  __shared__ __attribute__((aligned(16))) float sW[49 * kSgC * 4];  // [tap][o] float4
  for (int i = (int)threadIdx.x; i < 49 * kSgC; i += 256) {
    const int tap = i / kSgC, o = i - tap * kSgC;
    *reinterpret_cast<grad_f32x4*>(sW + (size_t)i * 4) = *reinterpret_cast<const grad_f32x4*>(Wp + (size_t)o * ldw + tap * 4);
  }
  __syncthreads();
  const int passes = (npix + kSgDgradPixels - 1) / kSgDgradPixels;
  for (int pass = (int)blockIdx.x; pass < passes; pass += (int)gridDim.x) {
    const int p = pass * kSgDgradPixels + (int)threadIdx.x;
    if (p >= npix) continue;
    const int ix = p % W, t = p / W;
    const int iy = t % H, b = t / H;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int ky = stem_first_tap(iy); ky < 7; ky += 2) {
      const int oy = stem_tap_source(iy, ky, oh);
      if (oy < 0) continue;
      for (int kx = stem_first_tap(ix); kx < 7; kx += 2) {
        const int ox = stem_tap_source(ix, kx, ow);
        if (ox < 0) continue;
        const float* g = dA + ((size_t)(b * oh + oy) * ow + ox) * kSgC;
        const float* w = sW + (size_t)(ky * 7 + kx) * kSgC * 4;
#pragma unroll 4
        for (int o4 = 0; o4 < kSgC; o4 += 4) {
          const grad_f32x4 gv = *reinterpret_cast<const grad_f32x4*>(g + o4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const grad_f32x4 wv = *reinterpret_cast<const grad_f32x4*>(w + (size_t)(o4 + e) * 4);
            const double gd = (double)gv[e];
            s0 = fma(gd, (double)wv.x, s0);
            s1 = fma(gd, (double)wv.y, s1);
            s2 = fma(gd, (double)wv.z, s2);
          }
        }
      }
    }
    const size_t plane = (size_t)H * W, at = (size_t)b * 3 * plane + (size_t)iy * W + ix;
    dx[at] = (float)s0;
    dx[at + plane] = (float)s1;
    dx[at + 2 * plane] = (float)s2;
  }
}

#undef GRAD_LANE_IDS

}  // namespace sfa
