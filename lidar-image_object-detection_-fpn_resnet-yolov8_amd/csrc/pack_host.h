// The host driver of the weight pack: sfa_pack_weights(_ex) (pack.hip) walks the pack units of pack_plan.h row by
// row with the element rules of pack_row.h, as the device kernel does (pack_kernel.h).  No HIP include:
// tools/pack_host_check.cpp runs the walk under ASan + UBSan.  clang only (pack_row.h).
#pragma once

#include "pack_plan.h"
#include "pack_row.h"

namespace sfa {

// The source table of a flat state: entry i of `layout` at its offset in `state` (the tensors back to back in
// layout order, the num_batches_tracked counters left out: null).
inline std::vector<const float*> pack_sources(const std::vector<Entry>& layout, const float* state) {
  std::vector<const float*> src;
  size_t off = 0;
  for (const Entry& e : layout) {
    src.push_back(is_batches_tracked(e) ? nullptr : state + off);
    if (!is_batches_tracked(e)) off += numel(e);
  }
  return src;
}

// One unit (one that pack_unit_fits): every row gathered in packed order with its BatchNorm scale folded in, rows
// [O, rows) and their b zero, then b, the bf16 terms, the fp16 terms and winv where the unit has them.
inline void pack_unit_host(const PackUnit& u, const float* const* src, float* packed) {
  uint16_t* wx = u.wx == kNoOffset ? nullptr : reinterpret_cast<uint16_t*>(packed + u.wx);
  uint16_t* wh = u.wh == kNoOffset ? nullptr : reinterpret_cast<uint16_t*>(packed + u.wh);
  const size_t plane = (size_t)u.N * u.Kpad;
  std::vector<float> row(u.Kpad);
  for (int r = 0; r < u.rows; ++r) {
    const int ph = r / u.N, n = r % u.N;  // PACK_CONV: ph = 0
    const int src_row = u.kind == PACK_DECONV ? n : r;
    const bool live = r < u.O;
    std::fill(row.begin(), row.end(), 0.f);
    double shift_sum = 0.0;
    for (int s = 0; live && s < u.nseg; ++s) {
      const PackSeg& sg = u.seg[s];
      double scale = 1.0;
      if (sg.bn[0] >= 0)
        scale = pack_bn_fold(src[sg.bn[0]][src_row], src[sg.bn[1]][src_row], src[sg.bn[2]][src_row],
                             src[sg.bn[3]][src_row], s, shift_sum);
      if (u.kind == PACK_DECONV) {
        for (int k = 0; k < 4 * sg.I; ++k)
          row[k] = (float)((double)src[sg.w][pack_deconv_src(ph, n, k, sg.I, u.N)] * scale);
      } else {
        const int taps = sg.KH * sg.KW;
        const float* w = src[sg.w] + (size_t)r * sg.I * taps;
        for (int c = 0; c < sg.I; ++c)
          for (int t = 0; t < taps; ++t) row[sg.k_off + t * sg.Cpad + c] = (float)((double)w[c * taps + t] * scale);
      }
    }
    std::copy(row.begin(), row.end(), packed + u.w + (size_t)r * u.Kpad);
    if (u.kind != PACK_DECONV || ph == 0)
      packed[u.b + src_row] = !live ? 0.f : u.bias >= 0 ? src[u.bias][src_row] : (float)shift_sum;
    const size_t term0 = (size_t)ph * 2 * plane + (size_t)n * u.Kpad;
    if (wx)
      for (int k = 0; k < u.Kpad; ++k) {
        uint32_t t[3];
        pack_bf16_terms(row[k], t);
        for (int q = 0; q < 3; ++q) wx[q * plane + term0 + k] = (uint16_t)t[q];
      }
    float mx = 0.f;
    for (int k = 0; k < u.Kpad; ++k) mx = std::max(mx, __builtin_fabsf(row[k]));
    const PackRowScale rs = pack_row_scale(mx);
    if (u.winv != kNoOffset) packed[u.winv + r] = rs.winv;
    if (wh)
      for (int k = 0; k < u.Kpad; ++k) {
        const PackHalfTerms h = pack_fp16_terms(row[k], rs.sc);
        wh[term0 + k] = (uint16_t)h.hi;
        wh[plane + term0 + k] = (uint16_t)h.lo;
      }
  }
}

// The whole pack: one zero fill (it is what leaves the alignment gaps zero), then every unit.
inline void pack_host(const std::vector<PackUnit>& units, const float* const* src, size_t total, float* packed) {
  std::fill(packed, packed + total, 0.f);
  for (const PackUnit& u : units) pack_unit_host(u, src, packed);
}

}  // namespace sfa
