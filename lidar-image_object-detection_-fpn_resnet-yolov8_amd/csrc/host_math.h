// Plain C++ integer helpers shared by the host code and the HIP units (no HIP include).
#pragma once

#include <cstddef>

namespace sfa {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

}  // namespace sfa
