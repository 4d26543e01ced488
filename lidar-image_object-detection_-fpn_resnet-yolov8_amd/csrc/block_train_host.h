// The launches of block_train_kernel.h's BatchNorm kernels (block_train.hip), for the entries that share them
// (block_train.hip, stem_train.hip): a __global__ function lives in one translation unit.  Maps are NHWC
// (npix, cout), cout a multiple of 4; sb = block_train_stat_blocks(npix, cout, cap).
#pragma once

#include "block_train_plan.h"
#include "common.h"

namespace sfa {

// stats [2][cout] = the batch mean and biased variance of z, coef [2][cout] = the float32 (s, t) of gamma, beta, eps;
// spart: float64 [sb.blocks][cout][2]
int launch_bn_train_stats(const GradBias& sb, const float* z, const float* gamma, const float* beta, double eps,
                          double* spart, float* stats, float* coef, hipStream_t st);

// out = max(fmaf(s, z, t) + skip, 0); skip: x (identity, zd null), fmaf(sd, zd, td) (zd and cd not null), or none
// (x and zd null)
int launch_bn_train_apply(int npix, int cout, const float* z, const float* coef, const float* x, const float* zd,
                          const float* cd, float* out, hipStream_t st);

// The backward of one BatchNorm over dY = g where gm > 0 (g itself when gm is null): dbeta, dgamma (each may be null)
// and, when dz is not null, dZ.  rpart: float64 [sb.blocks][cout][2], sums: float64 [cout][2]
int launch_bn_train_backward(const GradBias& sb, const float* g, const float* gm, const float* z, const float* stats,
                             const float* gamma, double eps, double* rpart, double* sums, float* dgamma, float* dbeta,
                             float* dz, hipStream_t st);

}  // namespace sfa
