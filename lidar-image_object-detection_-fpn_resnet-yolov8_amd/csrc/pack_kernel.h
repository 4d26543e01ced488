// The device form of sfa_pack_weights: one workgroup per packed row (pack_plan.h PackUnit). The row's source
// floats are read once, folded with the BatchNorm scale (double, as the host does) into an LDS row in packed
// order, reduced to the row maximum, and written out as f32, three bf16 terms, two scaled fp16 terms, winv and
// the bias. Every operation is the host's own (model.hip put_conv / bn_fold / split_terms / split_terms_h3), so
// the bytes are the host's: compiled with -ffp-contract=off.
#pragma once

#include "common.h"
#include "pack_plan.h"

namespace sfa {

constexpr int kPackThreads = 256;

struct PackSegDev {
  const float* w;
  const float* bn[4];  // gamma, beta, running_mean, running_var, or all null
  int I, KH, KW, Cpad, k_off;
};

struct PackUnitDev {
  PackSegDev seg[2];
  const float* bias;
  float* w;
  float* b;
  uint16_t* wx;
  uint16_t* wh;
  float* winv;
  int kind, O, rows, N, Kpad, nseg;
};

constexpr int kPackGaps = 16;
struct PackGapsDev {
  float* at[kPackGaps];
  int len[kPackGaps];
  int count;
};

// f32 -> bf16, round to nearest even, on the bits (finite inputs)
__device__ __forceinline__ uint32_t pack_bf16_rne(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

__device__ __forceinline__ uint32_t pack_half_bits(_Float16 h) {
  return (uint32_t) __builtin_bit_cast(unsigned short, h);
}

__global__ __launch_bounds__(kPackThreads) void pack_rows_kernel(const PackUnitDev u) {
  __shared__ float row[kPackMaxRow];
  __shared__ float wave_max[kPackThreads / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int ph = r / u.N, n = r % u.N;  // PACK_CONV: ph = 0
  const int src_row = u.kind == PACK_DECONV ? n : r;
  const bool live = r < u.O;

  for (int k = tid; k < u.Kpad; k += kPackThreads) row[k] = 0.f;
  __syncthreads();

  double shift_sum = 0.0;
  for (int s = 0; s < u.nseg; ++s) {
    const PackSegDev& sg = u.seg[s];
    double scale = 1.0;
    if (live && sg.bn[0]) {
      scale = (double)sg.bn[0][src_row] / sqrt((double)sg.bn[3][src_row] + 1e-5);
      const double shift = (double)sg.bn[1][src_row] - (double)sg.bn[2][src_row] * scale;
      shift_sum = s == 0 ? shift : shift_sum + shift;  // (a lone -0.0 shift stays -0.0)
    }
    if (!live) continue;
    if (u.kind == PACK_DECONV) {
      const int K = 4 * sg.I;
      for (int k = tid; k < K; k += kPackThreads)
        row[k] = (float)((double)sg.w[pack_deconv_src(ph, n, k, sg.I, u.N)] * scale);
    } else {
      const int taps = sg.KH * sg.KW, len = sg.I * taps;
      const float* src = sg.w + (size_t)r * len;
      for (int i = tid; i < len; i += kPackThreads) {
        const int c = i / taps, t = i - c * taps;
        row[sg.k_off + t * sg.Cpad + c] = (float)((double)src[i] * scale);
      }
    }
  }
  __syncthreads();

  float mx = 0.f;
  for (int k = tid; k < u.Kpad; k += kPackThreads) mx = fmaxf(mx, fabsf(row[k]));
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if ((tid & 63) == 0) wave_max[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));

  // e = floor(log2 max); a zero row keeps 13 (scale 1)
  int e = 13;
  if (mx > 0.f) {
    (void)frexpf(mx, &e);
    e -= 1;
  }
  const float sc = ldexpf(1.f, 13 - e);

  if (tid == 0) {
    if (u.winv) u.winv[r] = ldexpf(1.f, e - 13);
    if (u.kind != PACK_DECONV || ph == 0) {
      float b = 0.f;
      if (live) b = u.bias ? u.bias[src_row] : (float)shift_sum;
      u.b[src_row] = b;
    }
  }

  // eight elements per step: two 16-byte stores of f32, one 16-byte store per term
  const size_t plane = (size_t)u.N * u.Kpad;
  const size_t term0 = (size_t)ph * 2 * plane + (size_t)n * u.Kpad;
  float* wdst = u.w + (size_t)r * u.Kpad;
  for (int k = tid * 8; k < u.Kpad; k += kPackThreads * 8) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = row[k + j];
    *reinterpret_cast<float4*>(wdst + k) = make_float4(x[0], x[1], x[2], x[3]);
    *reinterpret_cast<float4*>(wdst + k + 4) = make_float4(x[4], x[5], x[6], x[7]);
    if (u.wx) {
      uint32_t t[3][8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = x[j];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          t[q][j] = pack_bf16_rne(v);
          v -= __uint_as_float(t[q][j] << 16);
        }
      }
#pragma unroll
      for (int q = 0; q < 3; ++q)
        *reinterpret_cast<uint4*>(u.wx + q * plane + term0 + k) =
            make_uint4(t[q][0] | (t[q][1] << 16), t[q][2] | (t[q][3] << 16), t[q][4] | (t[q][5] << 16),
                       t[q][6] | (t[q][7] << 16));
    }
    if (u.wh) {
      uint32_t hi[8], lo[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = x[j] * sc;
        const _Float16 h = (_Float16)v;
        const _Float16 l = (_Float16)(v - (float)h);
        hi[j] = pack_half_bits(h);
        lo[j] = pack_half_bits(l);
      }
      *reinterpret_cast<uint4*>(u.wh + term0 + k) =
          make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
      *reinterpret_cast<uint4*>(u.wh + plane + term0 + k) =
          make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
    }
  }
}

// The alignment gaps between packed regions, zero as the host's fill leaves them.
__global__ void pack_gaps_kernel(const PackGapsDev g) {
  for (int i = 0; i < g.count; ++i)
    for (int k = threadIdx.x; k < g.len[i]; k += blockDim.x) g.at[i][k] = 0.f;
}

}  // namespace sfa
