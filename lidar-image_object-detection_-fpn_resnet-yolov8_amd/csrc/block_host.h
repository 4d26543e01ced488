// The launches of block_kernel.h's gradient GEMMs (block.hip), for the entries that share them (block.hip,
// block_train.hip): a __global__ function lives in one translation unit.
#pragma once

#include "block_plan.h"
#include "common.h"

namespace sfa {

// out = the data gradient t describes: grid (grad_tiles(t.npix), t.cin / 64)
int launch_block_dgrad(const BkDgrad& t, float* out, hipStream_t st);

// dW (torch's (rows, cin, kh, kw)) = the weight gradient g of gr (masked by gm when it is not null) over x read at
// stride `stride` through taps tap0 .. tap0 + g.taps - 1: the split-K partials into `part`, then the shared fold
int launch_block_wgrad(const BlockWgrad& g, const BlockShape& s, const float* gr, const float* gm, const float* x, int h,
                       int w, int stride, int tap0, float* part, float* dW, hipStream_t st);

}  // namespace sfa
