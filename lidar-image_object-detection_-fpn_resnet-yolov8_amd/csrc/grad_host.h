// Host pieces the gradient operators' entries share (heads_grad.hip, neck.hip, block.hip, stem_grad.hip): the pointer
// checks, the refusal of a size query, and the launches of grad_common.hip.
#pragma once

#include <initializer_list>

#include "common.h"
#include "grad_plan.h"

namespace sfa {

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// every pointer of the list is 16-byte aligned (a null one is)
inline bool all_aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (!aligned16(p)) return false;
  return true;
}

// A size query (workspace_size, chunk_pixels) that refuses its arguments: the error text is set and 0 returned.
template <typename... A>
int refused(const char* fmt, A... args) {
  set_error(fmt, args...);
  return 0;
}

// db (b.cout) = the sum over the b.npix pixels of g (b.npix, b.cout), masked by gm (g where gm > 0) when it is not
// null: float64 sums over the plan's runs of pixels in pixel order into part [block][cout], then over the runs in run
// order, rounded once.
int launch_bias_grad(const GradBias& b, const float* g, const float* gm, double* part, float* db, hipStream_t st);

// dW[(o ldo + col0 + c) ntaps + tap] = the chunks of part[chunk][o][tap cin + c] (o < M) added in chunk order in
// float64, rounded once.  ldo = cin, col0 = 0: torch's (M, cin, kh, kw); ntaps = 1: columns col0 .. of a (M, ldo) matrix.
int launch_wgrad_fold(const float* part, int chunks, int M, int cin, int ntaps, float* dW, int ldo, int col0,
                      hipStream_t st);

}  // namespace sfa
