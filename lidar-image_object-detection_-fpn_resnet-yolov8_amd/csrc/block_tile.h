// The 64 x 64 tile pieces of the float32 MFMA gradient kernels (block_kernel.h, stem_grad_kernel.h) on
// v_mfma_f32_32x32x2_f32: a workgroup of 2 x 2 waves, one 16-register accumulator per wave, two k-major LDS tiles
// ([k][64], rows kBkLd words apart) walked in steps of kBkStep.
#pragma once

#include "block_plan.h"
#include "common.h"

namespace sfa {

typedef float bk_f32x16 __attribute__((ext_vector_type(16)));
typedef float bk_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBkLd = kBkTile + 4;  // words between two k rows of an LDS tile (neck_kernel.h kNkLd)
constexpr int kBkLdsWords = kBkStep * kBkLd;

__device__ __forceinline__ bk_f32x4 bk_zero4() { return bk_f32x4{0.f, 0.f, 0.f, 0.f}; }

// g where mask > 0 (strict, torch's ReLU backward), else 0
__device__ __forceinline__ bk_f32x4 bk_masked(bk_f32x4 g, bk_f32x4 m) {
  return bk_f32x4{m.x > 0.f ? g.x : 0.f, m.y > 0.f ? g.y : 0.f, m.z > 0.f ? g.z : 0.f, m.w > 0.f ? g.w : 0.f};
}

// the float4 at word `at` of g, masked by the same word of m when there is one
__device__ __forceinline__ bk_f32x4 bk_load_masked(const float* g, const float* m, size_t at) {
  const bk_f32x4 v = *reinterpret_cast<const bk_f32x4*>(g + at);
  return m ? bk_masked(v, *reinterpret_cast<const bk_f32x4*>(m + at)) : v;
}

// thread t holds the float4 of row t / 4, k-quad t % 4: stored transposed into a k-major tile
__device__ __forceinline__ void bk_store_kc(float* s, bk_f32x4 v, int tid) {
  float* d = s + (tid & 3) * 4 * kBkLd + (tid >> 2);
  d[0] = v.x, d[kBkLd] = v.y, d[2 * kBkLd] = v.z, d[3 * kBkLd] = v.w;
}

// thread t holds the float4 of k row t / 16, column quad t % 16: stored as it is
__device__ __forceinline__ void bk_store_mc(float* s, bk_f32x4 v, int tid) {
  *reinterpret_cast<bk_f32x4*>(s + (tid >> 4) * kBkLd + (tid & 15) * 4) = v;
}

// the step's 8 MFMAs of wave (wm, wn): rows wm * 32 .. of sA, columns wn * 32 .. of sB
__device__ __forceinline__ void bk_mma(const float* sA, const float* sB, int wm, int wn, int r, int hh, bk_f32x16& acc) {
  const float* A = sA + hh * kBkLd + wm * 32 + r;
  const float* Bp = sB + hh * kBkLd + wn * 32 + r;
#pragma unroll
  for (int s = 0; s < kBkStep / 2; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[2 * s * kBkLd], Bp[2 * s * kBkLd], acc, 0, 0, 0);
}

// row of accumulator register v inside the wave's 32 x 32 tile (the column is the lane's r)
__device__ __forceinline__ int bk_acc_row(int v, int hh) { return (v & 3) + 8 * (v >> 2) + 4 * hh; }

#define BK_LANE_IDS                                                 \
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;    \
  const int wm = wave & 1, wn = wave >> 1, r = lane & 31, hh = lane >> 5

// block.hip's launches that other operators share: db (block_bias_kernel + its fold) of a map g (b.npix, b.cout)
// masked by gm when it is not null, and the fold of a weight gradient's split-K partials into dW (g.rows, g.cin, g.taps).
int launch_block_bias_grad(const BlockBias& b, const float* g, const float* gm, double* part, float* db, hipStream_t st);
int launch_block_wgrad_fold(const BlockWgrad& g, const float* part, float* dW, hipStream_t st);

}  // namespace sfa
