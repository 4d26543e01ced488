// The 64 x 64 tile pieces of the float32 MFMA gradient kernels (neck_kernel.h, block_kernel.h, stem_grad_kernel.h) on
// v_mfma_f32_32x32x2_f32: a workgroup of 2 x 2 waves, one 16-register accumulator per wave, two k-major LDS tiles
// ([k][64], rows kGradLd words apart) walked in steps of kGradStep, so that lane (r, k) of the MFMA reads word r of
// row k for both operands.  A kernel that uses GRAD_LANE_IDS undefines it at its end.
#pragma once

#include "common.h"
#include "grad_plan.h"

namespace sfa {

typedef float grad_f32x16 __attribute__((ext_vector_type(16)));
typedef float grad_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGradLd = kGradTile + 4;  // words between two k rows of an LDS tile: the transposing stores of a wave
                                        // (4 k-quads x 16 rows) then fall on 64 different banks
constexpr int kGradLdsWords = kGradStep * kGradLd;

__device__ __forceinline__ grad_f32x4 grad_zero4() { return grad_f32x4{0.f, 0.f, 0.f, 0.f}; }

// g where mask > 0 (strict, torch's ReLU backward), else 0
__device__ __forceinline__ grad_f32x4 grad_masked(grad_f32x4 g, grad_f32x4 m) {
  return grad_f32x4{m.x > 0.f ? g.x : 0.f, m.y > 0.f ? g.y : 0.f, m.z > 0.f ? g.z : 0.f, m.w > 0.f ? g.w : 0.f};
}

// the float4 at word `at` of g, masked by the same word of m when there is one
__device__ __forceinline__ grad_f32x4 grad_load_masked(const float* g, const float* m, size_t at) {
  const grad_f32x4 v = *reinterpret_cast<const grad_f32x4*>(g + at);
  return m ? grad_masked(v, *reinterpret_cast<const grad_f32x4*>(m + at)) : v;
}

// 64 rows x kGradStep k of an operand whose rows are K-contiguous (row stride ld words): thread t loads the float4 at
// row t / 4, k-quad t % 4 (zero at and past `rows`) and stores it transposed into a k-major tile.
__device__ __forceinline__ grad_f32x4 grad_load_kc(const float* base, int ld, int row0, int rows, int k0, int tid) {
  const int m = tid >> 2, q4 = tid & 3;
  if (m >= rows) return grad_zero4();
  return *reinterpret_cast<const grad_f32x4*>(base + (size_t)(row0 + m) * ld + k0 + q4 * 4);
}
__device__ __forceinline__ void grad_store_kc(float* s, grad_f32x4 v, int tid) {
  float* d = s + (tid & 3) * 4 * kGradLd + (tid >> 2);
  d[0] = v.x, d[kGradLd] = v.y, d[2 * kGradLd] = v.z, d[3 * kGradLd] = v.w;
}

// kGradStep k x 64 columns of an operand that lies k-major (k row stride ld words): thread t loads the float4 at k row
// t / 16, column quad t % 16 (zero at and past `ks`) and stores it as it is.
__device__ __forceinline__ grad_f32x4 grad_load_mc(const float* base, int ld, int k0, int ks, int col0, int tid) {
  const int kk = tid >> 4, q4 = tid & 15;
  if (kk >= ks) return grad_zero4();
  return *reinterpret_cast<const grad_f32x4*>(base + (size_t)(k0 + kk) * ld + col0 + q4 * 4);
}
__device__ __forceinline__ void grad_store_mc(float* s, grad_f32x4 v, int tid) {
  *reinterpret_cast<grad_f32x4*>(s + (tid >> 4) * kGradLd + (tid & 15) * 4) = v;
}

// the step's 8 MFMAs of wave (wm, wn): rows wm * 32 .. of sA, columns wn * 32 .. of sB
__device__ __forceinline__ void grad_mma(const float* sA, const float* sB, int wm, int wn, int r, int hh, grad_f32x16& acc) {
  const float* A = sA + hh * kGradLd + wm * 32 + r;
  const float* Bp = sB + hh * kGradLd + wn * 32 + r;
#pragma unroll
  for (int s = 0; s < kGradStep / 2; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[2 * s * kGradLd], Bp[2 * s * kGradLd], acc, 0, 0, 0);
}

// row of accumulator register v inside the wave's 32 x 32 tile (the column is the lane's r)
__device__ __forceinline__ int grad_acc_row(int v, int hh) { return (v & 3) + 8 * (v >> 2) + 4 * hh; }

#define GRAD_LANE_IDS                                               \
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;    \
  const int wm = wave & 1, wn = wave >> 1, r = lane & 31, hh = lane >> 5

}  // namespace sfa
