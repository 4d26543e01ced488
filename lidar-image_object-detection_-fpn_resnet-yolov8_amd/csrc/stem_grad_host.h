// The launches of stem_grad_kernel.h's kernels (stem_grad.hip), for the entries that share them (stem_grad.hip,
// stem_train.hip): a __global__ function lives in one translation unit.
#pragma once

#include "common.h"
#include "stem_grad_plan.h"

namespace sfa {

// dA (npix_a, 64) = a > 0 ? pool adjoint of gp by first maximum : 0
int launch_stem_pool_adjoint(const StemShape& s, const float* a, const float* gp, float* dA, hipStream_t st);

// dW (64, 3, 7, 7) = wgrad_2(g, x): the split-K partials of g (npix_a, 64) over the NCHW image into `part`
// ([g.chunks][64][147]), then the shared fold
int launch_stem_wgrad(const BlockWgrad& g, const StemShape& s, const float* gr, const float* x, float* part, float* dW,
                      hipStream_t st);

// dx (B, 3, H, W) = dgrad_2(g; Wp), Wp rows [o][tap 4 + c] of ldw words
int launch_stem_dgrad(const StemShape& s, const float* gr, const float* Wp, int ldw, float* dx, hipStream_t st);

}  // namespace sfa
