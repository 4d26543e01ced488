// The device form of sfa_pack_weights: one workgroup per packed row (pack_plan.h PackUnit). The row's source
// floats are read once, folded with the BatchNorm scale (double, as the host does) into an LDS row in packed
// order, reduced to the row maximum, and written out as f32, three bf16 terms, two scaled fp16 terms, winv and
// the bias. The fold, the row exponent and the two splits are the functions of pack_row.h, the ones the host walk
// calls (pack_host.h), so the bytes are the host's: compiled with -ffp-contract=off.
#pragma once

#include "common.h"
#include "pack_plan.h"
#include "pack_row.h"

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
    if (live && sg.bn[0])
      scale = pack_bn_fold(sg.bn[0][src_row], sg.bn[1][src_row], sg.bn[2][src_row], sg.bn[3][src_row], s, shift_sum);
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

  const PackRowScale rs = pack_row_scale(mx);

  if (tid == 0) {
    if (u.winv) u.winv[r] = rs.winv;
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
        uint32_t tj[3];
        pack_bf16_terms(x[j], tj);
#pragma unroll
        for (int q = 0; q < 3; ++q) t[q][j] = tj[q];
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
        const PackHalfTerms h = pack_fp16_terms(x[j], rs.sc);
        hi[j] = h.hi;
        lo[j] = h.lo;
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
