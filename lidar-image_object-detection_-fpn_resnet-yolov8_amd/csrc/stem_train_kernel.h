// Kernels of sfa_stem_train_forward / sfa_stem_train_grad (gfx950): the stem (models/fpn_resnet.py:179-182) with bn1
// in training mode; stem_train_plan.h has the shapes.  Everything behind the convolution is launched through
// block_train_host.h (statistics, apply, BatchNorm backward), stem_grad_host.h (pool adjoint, dW, dx) and
// aux_kernels.h (max-pool).
//   stem_conv_fwd_kernel     z = conv7x7_2(x; W), no bias, no ReLU, float32: a forward implicit GEMM on grad_tile.h's
//                            64 x 64 tile (v_mfma_f32_32x32x2_f32): rows = 64 flat conv output pixels, columns = the 64
//                            output channels, K = the 147 (c, ky, kx) entries in torch's order padded to kStKPad, all
//                            of it inside one workgroup.  The A operand is gathered from the NCHW image: pixel (oy, ox)
//                            and entry (c, ky, kx) read x[b][c][2 oy - 3 + ky][2 ox - 3 + kx], zero outside the image
//                            (every row and column is tested) and at the padded entries; the B operand is the k-major
//                            copy [k][o] of W.
//   stem_w_relayout_kernel   torch's (64, 3, 7, 7) -> Wk [k][o] (k < kStKPad, zero rows past 146) and / or
//                            Wp [o][tap][4] = (c0, c1, c2, 0), the row order stem_dgrad_kernel reads
// No atomics; every sum has a fixed order, so runs are bit-identical.
#pragma once

#include "grad_tile.h"
#include "stem_train_plan.h"

namespace sfa {

// z[p][o] = sum over j = (c, ky, kx) of x[b][c][2 oy - 3 + ky][2 ox - 3 + kx] Wk[j][o], p = (b, oy, ox) flat.
// grid (grad_tiles(npix)), block (256)
__global__ void __launch_bounds__(256) stem_conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ Wk,
                                                            float* __restrict__ z, int H, int W, int oh, int ow,
                                                            int npix) {
  __shared__ __attribute__((aligned(16))) float sA[kGradLdsWords];
  __shared__ __attribute__((aligned(16))) float sB[kGradLdsWords];
  GRAD_LANE_IDS;
  const GradRange pt = grad_tile_at((int)blockIdx.x, npix);
  // this thread's A row: conv pixel pt.first + tid / 4, and its k quad of the step
  const int am = tid >> 2, aq = (tid & 3) * 4;
  const bool a_live = am < pt.count;
  int iy0 = 0, ix0 = 0;
  const float* xb = x;
  if (a_live) {
    const int p = pt.first + am;
    const int ox = p % ow, q = p / ow;
    const int oy = q % oh, b = q / oh;
    iy0 = 2 * oy - 3, ix0 = 2 * ox - 3;
    xb = x + (size_t)b * 3 * H * W;
  }
  const int bk = tid >> 4, bq = (tid & 15) * 4;  // this thread's B k row and column quad
  auto load_a = [&](int step) -> grad_f32x4 {
    grad_f32x4 v = grad_zero4();
    if (!a_live) return v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = step * kGradStep + aq + e;
      if (j < kStK) {
        int c, ky, kx;
        stem_column(j, &c, &ky, &kx);
        const int iy = iy0 + ky, ix = ix0 + kx;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v[e] = xb[((size_t)c * H + iy) * W + ix];
      }
    }
    return v;
  };
  auto load_b = [&](int step) -> grad_f32x4 {
    return *reinterpret_cast<const grad_f32x4*>(Wk + (size_t)(step * kGradStep + bk) * kSgC + bq);
  };
  grad_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  constexpr int steps = kStKPad / kGradStep;
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
  const int o = wn * 32 + r;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int q = wm * 32 + grad_acc_row(v, hh);
    if (q < pt.count) z[(size_t)(pt.first + q) * kSgC + o] = acc[v];
  }
}

// W (64, 3, 7, 7) as torch lays it -> Wk [k][o] (kStKPad rows) and Wp [o][tap][4], each skipped when null.
// grid (ceil(64 49 4 / 256)), block (256): thread e walks both copies (Wk has fewer words)
__global__ void __launch_bounds__(256) stem_w_relayout_kernel(const float* __restrict__ W, float* __restrict__ Wk,
                                                              float* __restrict__ Wp) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (Wk && e < kStKPad * kSgC) {
    const int k = e / kSgC, o = e - k * kSgC;
    Wk[e] = k < kStK ? W[(size_t)o * kStK + k] : 0.f;
  }
  if (Wp && e < kSgC * kStWpLd) {
    const int o = e / kStWpLd, rem = e - o * kStWpLd;
    const int tap = rem >> 2, c = rem & 3;
    Wp[e] = c < 3 ? W[(size_t)o * kStK + c * 49 + tap] : 0.f;
  }
}

#undef GRAD_LANE_IDS

}  // namespace sfa
