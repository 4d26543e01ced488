// Host-side dispatch: a runtime value becomes a compile-time one handed to a generic lambda, and a
// kernel launch returns its status.  A launch site reads
//   if (int rc = with_bool(raw, [&](auto RAW) { return launch({grid, block, st}, kernel<RAW.value>, args...); }))
//     return rc;
#pragma once

#include <type_traits>
#include <utility>

#include "common.h"
#include "conv_args.h"

namespace sfa {

template <int V>
using int_c = std::integral_constant<int, V>;

template <typename F>
int with_bool(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// the three layouts of the KITTI voxeliser (validated by the caller)
template <typename F>
int with_bev_layout(int layout, F&& f) {
  switch (layout) {
    case SFA_BEV_NCHW3_F32: return f(int_c<SFA_BEV_NCHW3_F32>{});
    case SFA_BEV_NCHW3_F64: return f(int_c<SFA_BEV_NCHW3_F64>{});
    default: return f(int_c<SFA_BEV_NHWC4_F32>{});
  }
}

// the two float32 layouts (the Argoverse kernels have no f64 form)
template <typename F>
int with_f32_layout(int layout, F&& f) {
  return layout == SFA_BEV_NHWC4_F32 ? f(int_c<SFA_BEV_NHWC4_F32>{}) : f(int_c<SFA_BEV_NCHW3_F32>{});
}

// the patch stem's three input layouts (conv_args.h StemInput)
template <typename F>
int with_stem_in(int stem_in, F&& f) {
  switch (stem_in) {
    case STEM_IN_NCHW3: return f(int_c<STEM_IN_NCHW3>{});
    case STEM_IN_NCHW3_FLIP: return f(int_c<STEM_IN_NCHW3_FLIP>{});
    default: return f(int_c<STEM_IN_NHWC4>{});
  }
}

struct LaunchCfg {
  dim3 grid, block;
  hipStream_t st;
  const char* file;
  int line;
  LaunchCfg(dim3 g, dim3 b, hipStream_t s, const char* f = __builtin_FILE(), int l = __builtin_LINE())
      : grid(g), block(b), st(s), file(f), line(l) {}
};

// Enqueues the kernel and checks the launch (configuration errors only; no sync): SFA_OK or SFA_E_HIP.
template <typename... P, typename... A>
int launch(const LaunchCfg& c, void (*kernel)(P...), A&&... args) {
  kernel<<<c.grid, c.block, 0, c.st>>>(std::forward<A>(args)...);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return SFA_OK;
  set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e), c.file, c.line);
  return SFA_E_HIP;
}

}  // namespace sfa
