// apply_kfpn as an operator of its own, forward and gradient (gfx950): replaces, for a detector built in
// torch, models/fpn_resnet.py:248-254 apply_kfpn with the nearest resize of level 0 (:229-230) and the
// autograd graph behind them.  The model's forward keeps its fused kfpn_combine_kernel (aux_kernels.hip);
// kfpn_fwd_kernel repeats that kernel's rounding sequence on the user-facing layouts.
//
//   kfpn_fwd_kernel    per element: max, three expf(v - mx), the sum, three divisions, v0 w0 + v1 w1 + v2 w2
//                      in float32 without contraction; optionally the weights (B, c, h, w, 3)
//   kfpn_grad_kernel   d total / d v_j = g w_j (1 + v_j - out) in float64 from the float32 operands, rounded
//                      once; level 0 at half resolution gathers its four children in the fixed order
//                      (0,0), (0,1), (1,0), (1,1): no atomics, every gradient byte written, runs bit-identical
//
// Both cover all heads in one launch: grid (pixel chunk, frame, concatenated channel), the heads' pointers in
// a by-value table.  The vector instantiations move 128 bits per load / store (w % 4 == 0 and every base
// 16-byte aligned); the scalar ones give each thread the same elements and the same arithmetic, and no sum
// crosses a thread, so the bits do not depend on the form.
#include <math.h>

#include "dispatch.h"

#pragma clang fp contract(off)

namespace sfa {

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;  // pixels of one thread (forward, full-resolution gradient); a 4 x 2 block under level0_half

// Head j owns the concatenated channels [off[j], off[j] + ch[j]); its maps are NCHW (B, ch[j], h, w).
struct KfpnHeads {
  const float* lv[SFA_MAX_HEADS][3];
  int ch[SFA_MAX_HEADS];
  int off[SFA_MAX_HEADS];
  int num_heads;
};

struct KfpnFwdOut {
  float* out[SFA_MAX_HEADS];
  float* wts[SFA_MAX_HEADS];  // null: not wanted
};

struct KfpnGradIo {
  const float* g[SFA_MAX_HEADS];
  float* gl[SFA_MAX_HEADS][3];
};

__device__ __forceinline__ int head_of(const KfpnHeads& t, int cc) {
  int hd = 0;
#pragma unroll
  for (int j = 1; j < SFA_MAX_HEADS; ++j)
    if (j < t.num_heads && cc >= t.off[j]) hd = j;
  return hd;
}

// kfpn_combine_kernel's sequence (torch's softmax: max-subtract, exp, sum, divide), one element
__device__ __forceinline__ float combine_f32(float v0, float v1, float v2, float wt[3]) {
  const float mx = fmaxf(fmaxf(v0, v1), v2);
  const float e0 = expf(v0 - mx), e1 = expf(v1 - mx), e2 = expf(v2 - mx);
  const float sum = e0 + e1 + e2;
  wt[0] = e0 / sum;
  wt[1] = e1 / sum;
  wt[2] = e2 / sum;
  return v0 * wt[0] + v1 * wt[1] + v2 * wt[2];
}

// grid (ceil(h w / 4 / 256), B, channels of all heads); pixels p .. p + 3 of the flat map per thread
template <bool VEC, bool HALF>
__global__ void __launch_bounds__(kThreads) kfpn_fwd_kernel(KfpnHeads t, KfpnFwdOut o, int h, int w) {
  const int hw = h * w;
  const int p = ((int)blockIdx.x * kThreads + (int)threadIdx.x) * kPix;
  if (p >= hw) return;
  const int b = blockIdx.y, cc = blockIdx.z;
  const int hd = head_of(t, cc);
  const size_t plane = (size_t)b * t.ch[hd] + (cc - t.off[hd]);
  const int w0 = w / 2;
  const float* L0 = t.lv[hd][0] + plane * (HALF ? (size_t)(h / 2) * w0 : (size_t)hw);
  const float* L1 = t.lv[hd][1] + plane * hw;
  const float* L2 = t.lv[hd][2] + plane * hw;
  const int np = VEC ? kPix : (hw - p < kPix ? hw - p : kPix);
  float a0[kPix] = {0.f, 0.f, 0.f, 0.f}, a1[kPix] = {0.f, 0.f, 0.f, 0.f}, a2[kPix] = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    // w % 4 == 0: the four pixels share a row; under HALF they read level-0 columns xx / 2, xx / 2 + 1
    const float4 l1 = *reinterpret_cast<const float4*>(L1 + p);
    const float4 l2 = *reinterpret_cast<const float4*>(L2 + p);
    a1[0] = l1.x, a1[1] = l1.y, a1[2] = l1.z, a1[3] = l1.w;
    a2[0] = l2.x, a2[1] = l2.y, a2[2] = l2.z, a2[3] = l2.w;
    if (HALF) {
      const int yy = p / w, xx = p - yy * w;
      const float2 l0 = *reinterpret_cast<const float2*>(L0 + (yy >> 1) * w0 + (xx >> 1));
      a0[0] = l0.x, a0[1] = l0.x, a0[2] = l0.y, a0[3] = l0.y;
    } else {
      const float4 l0 = *reinterpret_cast<const float4*>(L0 + p);
      a0[0] = l0.x, a0[1] = l0.y, a0[2] = l0.z, a0[3] = l0.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      if (i >= np) break;
      const int q = p + i, yy = q / w, xx = q - yy * w;
      a0[i] = HALF ? L0[(yy >> 1) * w0 + (xx >> 1)] : L0[q];
      a1[i] = L1[q];
      a2[i] = L2[q];
    }
  }
  float r[kPix], wt[kPix][3];
#pragma unroll
  for (int i = 0; i < kPix; ++i) r[i] = combine_f32(a0[i], a1[i], a2[i], wt[i]);
  float* out = o.out[hd] + plane * hw + p;
  float* wts = o.wts[hd];
  if (VEC) {
    *reinterpret_cast<float4*>(out) = make_float4(r[0], r[1], r[2], r[3]);
    if (wts) {
      float4* dst = reinterpret_cast<float4*>(wts + (plane * hw + p) * 3);
      dst[0] = make_float4(wt[0][0], wt[0][1], wt[0][2], wt[1][0]);
      dst[1] = make_float4(wt[1][1], wt[1][2], wt[2][0], wt[2][1]);
      dst[2] = make_float4(wt[2][2], wt[3][0], wt[3][1], wt[3][2]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      if (i >= np) break;
      out[i] = r[i];
      if (wts) {
        float* dst = wts + (plane * hw + p + i) * 3;
        dst[0] = wt[i][0], dst[1] = wt[i][1], dst[2] = wt[i][2];
      }
    }
  }
}

// The three terms g w_j (1 + v_j - out) of one element, float64 from the float32 operands.
__device__ __forceinline__ void grad_terms(float f0, float f1, float f2, float fg, double d[3]) {
  const double v0 = (double)f0, v1 = (double)f1, v2 = (double)f2, g = (double)fg;
  const double mx = fmax(fmax(v0, v1), v2);
  const double e0 = exp(v0 - mx), e1 = exp(v1 - mx), e2 = exp(v2 - mx);
  const double sum = e0 + e1 + e2;
  const double w0 = e0 / sum, w1 = e1 / sum, w2 = e2 / sum;
  const double out = v0 * w0 + v1 * w1 + v2 * w2;
  d[0] = g * w0 * (1 + v0 - out);
  d[1] = g * w1 * (1 + v1 - out);
  d[2] = g * w2 * (1 + v2 - out);
}

// HALF: grid (ceil(h0 w0 / 2 / 256), B, channels); a thread owns the level-0 cells k, k + 1 of the flat
// (h0, w0) map and their 2 x 2 children: it writes those cells' level-0 gradient (the adjoint of the nearest
// resize as a gather) and the children's level-1 and level-2 gradients.  In the vector form (w0 even) the
// two cells share a row, and the eight children are columns 2 cx .. 2 cx + 3 of rows 2 cy, 2 cy + 1.
// Not HALF: grid (ceil(h w / 4 / 256), B, channels), pixels p .. p + 3, all three levels element-wise.
template <bool VEC, bool HALF>
__global__ void __launch_bounds__(kThreads) kfpn_grad_kernel(KfpnHeads t, KfpnGradIo io, int h, int w) {
  const int hw = h * w;
  const int b = blockIdx.y, cc = blockIdx.z;
  const int first = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if constexpr (HALF) {
    const int w0 = w / 2, n0 = (h / 2) * w0;
    const int k = first * 2;
    if (k >= n0) return;
    const int hd = head_of(t, cc);
    const size_t plane = (size_t)b * t.ch[hd] + (cc - t.off[hd]);
    const float* L0 = t.lv[hd][0] + plane * n0;
    const float* L1 = t.lv[hd][1] + plane * hw;
    const float* L2 = t.lv[hd][2] + plane * hw;
    const float* G = io.g[hd] + plane * hw;
    float* G0 = io.gl[hd][0] + plane * n0;
    float* G1 = io.gl[hd][1] + plane * hw;
    float* G2 = io.gl[hd][2] + plane * hw;
    const int nc = VEC ? 2 : (n0 - k < 2 ? n0 - k : 2);
    // [row of the 2 x 2 block][2 * cell + column of the block]
    float l0[2] = {0.f, 0.f}, l1[2][4], l2[2][4], gg[2][4], o1[2][4], o2[2][4], o0[2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) l1[r][c] = l2[r][c] = gg[r][c] = 0.f;
    if (VEC) {
      const int cy = k / w0, cx = k - cy * w0;
      const float2 a = *reinterpret_cast<const float2*>(L0 + k);
      l0[0] = a.x, l0[1] = a.y;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int q = (2 * cy + r) * w + 2 * cx;
        const float4 x1 = *reinterpret_cast<const float4*>(L1 + q);
        const float4 x2 = *reinterpret_cast<const float4*>(L2 + q);
        const float4 xg = *reinterpret_cast<const float4*>(G + q);
        l1[r][0] = x1.x, l1[r][1] = x1.y, l1[r][2] = x1.z, l1[r][3] = x1.w;
        l2[r][0] = x2.x, l2[r][1] = x2.y, l2[r][2] = x2.z, l2[r][3] = x2.w;
        gg[r][0] = xg.x, gg[r][1] = xg.y, gg[r][2] = xg.z, gg[r][3] = xg.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j >= nc) break;
        const int cy = (k + j) / w0, cx = (k + j) - cy * w0;
        l0[j] = L0[k + j];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int q = (2 * cy + r) * w + 2 * cx + c;
            l1[r][2 * j + c] = L1[q];
            l2[r][2 * j + c] = L2[q];
            gg[r][2 * j + c] = G[q];
          }
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      double acc = 0;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {  // children (0,0), (0,1), (1,0), (1,1)
          double d[3];
          grad_terms(l0[j], l1[r][2 * j + c], l2[r][2 * j + c], gg[r][2 * j + c], d);
          acc += d[0];
          o1[r][2 * j + c] = (float)d[1];
          o2[r][2 * j + c] = (float)d[2];
        }
      o0[j] = (float)acc;
    }
    if (VEC) {
      const int cy = k / w0, cx = k - cy * w0;
      *reinterpret_cast<float2*>(G0 + k) = make_float2(o0[0], o0[1]);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int q = (2 * cy + r) * w + 2 * cx;
        *reinterpret_cast<float4*>(G1 + q) = make_float4(o1[r][0], o1[r][1], o1[r][2], o1[r][3]);
        *reinterpret_cast<float4*>(G2 + q) = make_float4(o2[r][0], o2[r][1], o2[r][2], o2[r][3]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j >= nc) break;
        const int cy = (k + j) / w0, cx = (k + j) - cy * w0;
        G0[k + j] = o0[j];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int q = (2 * cy + r) * w + 2 * cx + c;
            G1[q] = o1[r][2 * j + c];
            G2[q] = o2[r][2 * j + c];
          }
      }
    }
  } else {
    const int p = first * kPix;
    if (p >= hw) return;
    const int hd = head_of(t, cc);
    const size_t base = ((size_t)b * t.ch[hd] + (cc - t.off[hd])) * hw + p;
    const float* L0 = t.lv[hd][0] + base;
    const float* L1 = t.lv[hd][1] + base;
    const float* L2 = t.lv[hd][2] + base;
    const float* G = io.g[hd] + base;
    const int np = VEC ? kPix : (hw - p < kPix ? hw - p : kPix);
    float a[4][kPix], r[3][kPix];
#pragma unroll
    for (int i = 0; i < kPix; ++i) a[0][i] = a[1][i] = a[2][i] = a[3][i] = 0.f;
    if (VEC) {
      const float4 x0 = *reinterpret_cast<const float4*>(L0), x1 = *reinterpret_cast<const float4*>(L1);
      const float4 x2 = *reinterpret_cast<const float4*>(L2), xg = *reinterpret_cast<const float4*>(G);
      a[0][0] = x0.x, a[0][1] = x0.y, a[0][2] = x0.z, a[0][3] = x0.w;
      a[1][0] = x1.x, a[1][1] = x1.y, a[1][2] = x1.z, a[1][3] = x1.w;
      a[2][0] = x2.x, a[2][1] = x2.y, a[2][2] = x2.z, a[2][3] = x2.w;
      a[3][0] = xg.x, a[3][1] = xg.y, a[3][2] = xg.z, a[3][3] = xg.w;
    } else {
#pragma unroll
      for (int i = 0; i < kPix; ++i) {
        if (i >= np) break;
        a[0][i] = L0[i], a[1][i] = L1[i], a[2][i] = L2[i], a[3][i] = G[i];
      }
    }
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      double d[3];
      grad_terms(a[0][i], a[1][i], a[2][i], a[3][i], d);
      r[0][i] = (float)d[0], r[1][i] = (float)d[1], r[2][i] = (float)d[2];
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      float* dst = io.gl[hd][l] + base;
      if (VEC) {
        *reinterpret_cast<float4*>(dst) = make_float4(r[l][0], r[l][1], r[l][2], r[l][3]);
      } else {
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
          if (i >= np) break;
          dst[i] = r[l][i];
        }
      }
    }
  }
}

struct KfpnShape {
  int total_ch;
  bool vec;  // so far: w % 4 == 0 and the level pointers 16-byte aligned; the entry adds its own buffers
};

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// The checks both entries share, before any launch; fills the table's level pointers, channels and offsets.
int kfpn_check(const char* who, const float* const* levels, const int* channels, int num_heads, int B, int h, int w,
               int level0_half, KfpnHeads* t, KfpnShape* s) {
  SFA_CHECK_ARG(levels, "%s: null levels", who);
  SFA_CHECK_ARG(channels, "%s: null channels", who);
  SFA_CHECK_ARG(num_heads >= 1 && num_heads <= SFA_MAX_HEADS, "%s: num_heads %d outside 1..%d", who, num_heads,
                SFA_MAX_HEADS);
  SFA_CHECK_ARG(B > 0, "%s: B %d must be positive", who, B);
  SFA_CHECK_ARG(h > 0 && w > 0, "%s: h %d, w %d must be positive", who, h, w);
  SFA_CHECK_ARG(level0_half == 0 || level0_half == 1, "%s: level0_half %d is not 0 or 1", who, level0_half);
  SFA_CHECK_ARG(!level0_half || (h % 2 == 0 && w % 2 == 0), "%s: level0_half needs even h and w, got %d x %d", who, h,
                w);
  SFA_CHECK_ARG((int64_t)h * w <= (int64_t)1 << 30, "%s: h x w = %d x %d above 2^30 cells (32-bit pixel index)", who, h,
                w);
  int64_t total = 0;
  s->vec = w % 4 == 0;
  t->num_heads = num_heads;
  for (int j = 0; j < SFA_MAX_HEADS; ++j) {
    t->ch[j] = t->off[j] = 0;
    for (int l = 0; l < 3; ++l) t->lv[j][l] = nullptr;
  }
  for (int j = 0; j < num_heads; ++j) {
    SFA_CHECK_ARG(channels[j] > 0, "%s: channels[%d] = %d must be positive", who, j, channels[j]);
    t->ch[j] = channels[j];
    t->off[j] = (int)total;
    total += channels[j];
    SFA_CHECK_ARG(total <= 65535, "%s: channels sum above 65535 (grid z limit)", who);
    for (int l = 0; l < 3; ++l) {
      SFA_CHECK_ARG(levels[3 * j + l], "%s: null levels[%d] (head %d, level %d)", who, 3 * j + l, j, l);
      t->lv[j][l] = levels[3 * j + l];
      s->vec = s->vec && aligned16(levels[3 * j + l]);
    }
  }
  SFA_CHECK_ARG(B <= 65535, "%s: B %d above 65535 (grid y limit)", who, B);
  s->total_ch = (int)total;
  return SFA_OK;
}

}  // namespace

}  // namespace sfa

using namespace sfa;

extern "C" int sfa_kfpn_combine(const float* const* levels, const int* channels, int num_heads, int B, int h, int w,
                                int level0_half, float* const* out, float* const* weights, void* stream) {
  KfpnHeads t;
  KfpnShape s;
  if (int rc = kfpn_check("kfpn_combine", levels, channels, num_heads, B, h, w, level0_half, &t, &s)) return rc;
  SFA_CHECK_ARG(out, "kfpn_combine: null out");
  KfpnFwdOut o;
  for (int j = 0; j < SFA_MAX_HEADS; ++j) o.out[j] = o.wts[j] = nullptr;
  for (int j = 0; j < num_heads; ++j) {
    SFA_CHECK_ARG(out[j], "kfpn_combine: null out[%d]", j);
    SFA_CHECK_ARG(!weights || weights[j], "kfpn_combine: null weights[%d]", j);
    o.out[j] = out[j];
    o.wts[j] = weights ? weights[j] : nullptr;
    s.vec = s.vec && aligned16(o.out[j]) && aligned16(o.wts[j]);
  }
  const dim3 grid((unsigned)ceil_div(ceil_div(h * w, kPix), kThreads), (unsigned)B, (unsigned)s.total_ch);
  return with_bool(s.vec, [&](auto VEC) {
    return with_bool(level0_half != 0, [&](auto HALF) {
      return launch({grid, dim3(kThreads), reinterpret_cast<hipStream_t>(stream)},
                    kfpn_fwd_kernel<VEC.value, HALF.value>, t, o, h, w);
    });
  });
}

extern "C" int sfa_kfpn_combine_grad(const float* const* levels, const int* channels, int num_heads, int B, int h,
                                     int w, int level0_half, const float* const* grad_out,
                                     float* const* grad_levels, void* stream) {
  KfpnHeads t;
  KfpnShape s;
  if (int rc = kfpn_check("kfpn_combine_grad", levels, channels, num_heads, B, h, w, level0_half, &t, &s)) return rc;
  SFA_CHECK_ARG(grad_out, "kfpn_combine_grad: null grad_out");
  SFA_CHECK_ARG(grad_levels, "kfpn_combine_grad: null grad_levels");
  KfpnGradIo io;
  for (int j = 0; j < SFA_MAX_HEADS; ++j) {
    io.g[j] = nullptr;
    for (int l = 0; l < 3; ++l) io.gl[j][l] = nullptr;
  }
  for (int j = 0; j < num_heads; ++j) {
    SFA_CHECK_ARG(grad_out[j], "kfpn_combine_grad: null grad_out[%d]", j);
    io.g[j] = grad_out[j];
    s.vec = s.vec && aligned16(io.g[j]);
    for (int l = 0; l < 3; ++l) {
      SFA_CHECK_ARG(grad_levels[3 * j + l], "kfpn_combine_grad: null grad_levels[%d] (head %d, level %d)", 3 * j + l,
                    j, l);
      io.gl[j][l] = grad_levels[3 * j + l];
      s.vec = s.vec && aligned16(io.gl[j][l]);
    }
  }
  // threads of one (frame, channel): pairs of level-0 cells, or quads of pixels
  const int units = level0_half ? ceil_div((h / 2) * (w / 2), 2) : ceil_div(h * w, kPix);
  const dim3 grid((unsigned)ceil_div(units, kThreads), (unsigned)B, (unsigned)s.total_ch);
  return with_bool(s.vec, [&](auto VEC) {
    return with_bool(level0_half != 0, [&](auto HALF) {
      return launch({grid, dim3(kThreads), reinterpret_cast<hipStream_t>(stream)},
                    kfpn_grad_kernel<VEC.value, HALF.value>, t, io, h, w);
    });
  });
}
