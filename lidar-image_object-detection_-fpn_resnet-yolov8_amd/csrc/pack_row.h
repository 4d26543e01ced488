// The element rules of the weight pack, once: the BatchNorm fold of one row, the row exponent of the fp16x3 form,
// the three bf16 terms and the two scaled fp16 terms of one float.  The host walk (pack_host.h) and the device
// kernel (pack_kernel.h) both call these four functions, so the bytes of the two are one definition.  b - mu * scale
// and x * sc - hi stay two roundings on every target: contraction is off inside the two functions that hold them
// (and pack.hip is compiled with -ffp-contract=off).  Builtins only, the same on both sides; _Float16: clang, not
// g++ on x86.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SFA_PACK_FN __host__ __device__ inline
#else
#define SFA_PACK_FN inline
#endif

namespace sfa {

// One row of segment s of a unit: returns scale = gamma / sqrt(var + 1e-5) and adds shift = beta - mu * scale to the
// unit's sum, all in double.  The first segment's shift starts the sum (a lone -0.0 shift stays -0.0).
SFA_PACK_FN double pack_bn_fold(float g, float b, float mu, float var, int s, double& shift_sum) {
#pragma clang fp contract(off)
  const double scale = (double)g / __builtin_sqrt((double)var + 1e-5);
  const double shift = (double)b - (double)mu * scale;
  shift_sum = s == 0 ? shift : shift_sum + shift;
  return scale;
}

// fp16x3 scale of a row whose largest |element| is mx: e = floor(log2 mx), a zero row keeps e = 13 (scale 1);
// sc = 2^(13 - e) brings every |element| below 2^14, winv = 2^(e - 13) undoes it.
struct PackRowScale {
  float sc, winv;
};
SFA_PACK_FN PackRowScale pack_row_scale(float mx) {
  int e = 13;
  if (mx > 0.f) {
    (void)__builtin_frexpf(mx, &e);  // mx in [2^(e-1), 2^e)
    e -= 1;
  }
  return {__builtin_ldexpf(1.f, 13 - e), __builtin_ldexpf(1.f, e - 13)};
}

// x -> three bf16 terms t0 + t1 + t2 == x: f32 -> bf16 rounds to nearest even on the bits (finite inputs), each
// residual is subtracted in float (and is exact there).
SFA_PACK_FN void pack_bf16_terms(float x, uint32_t t[3]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    u += 0x7fffu + ((u >> 16) & 1u);
    t[q] = u >> 16;
    x -= __builtin_bit_cast(float, t[q] << 16);
  }
}

// x * sc = hi + lo with hi = fp16(x * sc) and lo = fp16(x * sc - hi), as bits (fp16 subnormals are kept).
struct PackHalfTerms {
  uint32_t hi, lo;
};
SFA_PACK_FN PackHalfTerms pack_fp16_terms(float x, float sc) {
#pragma clang fp contract(off)
  const float v = x * sc;
  const _Float16 hi = (_Float16)v;
  const _Float16 lo = (_Float16)(v - (float)hi);
  return {(uint32_t) __builtin_bit_cast(unsigned short, hi), (uint32_t) __builtin_bit_cast(unsigned short, lo)};
}

}  // namespace sfa
