// Stand-alone run of the host weight pack (csrc/pack_host.h over the units of csrc/pack_plan.h with the rules of
// csrc/pack_row.h), the walk sfa_pack_weights(_ex) makes, under ASan + UBSan.  Per head set and family: a
// deterministic finite state with positive running_var, every tensor an allocation of its own (a source index
// outside a tensor is an ASan report); every unit passes pack_unit_fits; a unit-by-unit pass into a buffer of 0xFF
// bytes, without the zero fill, leaves no destination region unwritten and writes nothing outside the regions; the
// whole pack (pack_host: zero fill, then the units) gives the same regions, zero gaps, finite floats and finite
// terms everywhere, and every winv a power of two.  Head sets come from the command line (pack_check_sets.h).
// clang only (_Float16):
//   clang++ -std=c++17 -O2 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//     tools/pack_host_check.cpp -o /tmp/pack_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/pack_host.h"
#include "pack_check_sets.h"
#include "plan_check.h"

using namespace sfa;

// a counter hash to [-0.5, 0.5)
static float fill_value(uint32_t tensor, uint32_t i) {
  uint32_t x = tensor * 0x9E3779B9u + i * 0x85EBCA6Bu + 0x27D4EB2Fu;
  x ^= x >> 16, x *= 0x7FEB352Du, x ^= x >> 15, x *= 0x846CA68Bu, x ^= x >> 16;
  return (float)(x >> 8) * (1.f / 16777216.f) - 0.5f;
}

static bool ends_with(const std::string& s, const char* tail) {
  const size_t n = strlen(tail);
  return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}

static uint32_t word(const float* p) { return __builtin_bit_cast(uint32_t, *p); }

static void check_family(const char* what, const sfa_arch* a, int backbone) {
  const std::vector<Entry> layout = state_layout(a, backbone);
  const std::vector<PackUnit> units = pack_units(a, backbone);
  const size_t total = make_plan(a, backbone).total;
  ++plans;
  for (const PackUnit& u : units)
    if (!pack_unit_fits(u, layout)) {
      EXPECT(false, "%s: a unit of %d rows x %d does not fit the drivers", what, u.rows, u.Kpad);
      return;
    }

  std::vector<std::vector<float>> tensors(layout.size());
  std::vector<const float*> src(layout.size(), nullptr);
  for (size_t t = 0; t < layout.size(); ++t) {
    if (is_batches_tracked(layout[t])) continue;
    tensors[t].resize((size_t)numel(layout[t]));
    const bool var = ends_with(layout[t].name, "running_var");
    for (size_t i = 0; i < tensors[t].size(); ++i) {
      const float v = fill_value((uint32_t)t, (uint32_t)i);
      tensors[t][i] = var ? 0.5f + std::fabs(v) : v;
    }
    src[t] = tensors[t].data();
  }

  // unit by unit into 0xFF bytes, no zero fill
  std::vector<float> units_only(total), whole(total);
  memset(units_only.data(), 0xFF, total * sizeof(float));
  for (const PackUnit& u : units) pack_unit_host(u, src.data(), units_only.data());
  memset(whole.data(), 0xFF, total * sizeof(float));
  pack_host(units, src.data(), total, whole.data());

  for (const PackUnit& u : units)
    for (const auto& r : pack_unit_regions(u)) {
      const bool f32 = r.first == u.w || r.first == u.b || r.first == u.winv;
      size_t unwritten = 0, not_finite = 0;
      for (size_t i = r.first; i < r.second; ++i) {
        const uint32_t w = word(&units_only[i]);
        if (f32) {
          unwritten += w == 0xFFFFFFFFu;
          not_finite += !std::isfinite(units_only[i]);
        } else {  // two bf16 or fp16 terms: 0xFFFF is a NaN in both formats
          unwritten += (w & 0xFFFFu) == 0xFFFFu || (w >> 16) == 0xFFFFu;
          const bool bf16 = u.wx != kNoOffset && r.first >= u.wx && (u.wh == kNoOffset || r.first < u.wh);
          const uint32_t exp_mask = bf16 ? 0x7F80u : 0x7C00u;
          not_finite += ((w & exp_mask) == exp_mask) || (((w >> 16) & exp_mask) == exp_mask);
        }
      }
      EXPECT(unwritten == 0, "%s: %zu unwritten values in region [%zu, %zu)", what, unwritten, r.first, r.second);
      EXPECT(not_finite == 0, "%s: %zu values not finite in region [%zu, %zu)", what, not_finite, r.first, r.second);
      EXPECT(memcmp(&units_only[r.first], &whole[r.first], (r.second - r.first) * sizeof(float)) == 0,
             "%s: region [%zu, %zu) differs between the unit pass and the whole pack", what, r.first, r.second);
    }
  for (const PackUnit& u : units) {
    if (u.winv == kNoOffset) continue;
    size_t not_pow2 = 0;
    for (int r = 0; r < u.rows; ++r) {
      int e;
      const float v = whole[u.winv + r];
      not_pow2 += !(v > 0.f && std::frexp(v, &e) == 0.5f);
    }
    EXPECT(not_pow2 == 0, "%s: %zu winv of the unit at %zu are no power of two", what, not_pow2, u.w);
  }
  for (const auto& g : pack_gaps(units, total)) {
    size_t touched = 0, not_zero = 0;
    for (size_t i = g.first; i < g.second; ++i) {
      touched += word(&units_only[i]) != 0xFFFFFFFFu;
      not_zero += word(&whole[i]) != 0;
    }
    EXPECT(touched == 0, "%s: a unit wrote %zu floats of the gap [%zu, %zu)", what, touched, g.first, g.second);
    EXPECT(not_zero == 0, "%s: %zu floats of the gap [%zu, %zu) are not zero", what, not_zero, g.first, g.second);
  }
  size_t not_finite = 0;
  for (size_t i = 0; i < total; ++i) not_finite += !std::isfinite(whole[i]);
  EXPECT(not_finite == 0, "%s: %zu floats of the packed buffer are not finite", what, not_finite);
}

int main(int argc, char** argv) {
  const std::vector<std::string> sets = sets_of(argc, argv);
  for (const std::string& s : sets) {
    sfa_arch a;
    if (!parse_set(s.c_str(), &a)) {
      std::printf("cannot parse head set %s\n", s.c_str());
      return 2;
    }
    check_family(("fpn_resnet_18 " + s).c_str(), &a, SFA_BACKBONE_KFPN);
    check_family(("resnet_18 " + s).c_str(), &a, SFA_BACKBONE_DECONV);
  }
  std::printf("%zu head sets, %ld packs, %ld bad\n", sets.size(), plans, bad);
  return bad ? 1 : 0;
}
