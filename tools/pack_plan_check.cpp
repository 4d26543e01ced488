// Stand-alone check of the weight-pack plan (csrc/pack_plan.h), host only: the pack units of both families
// against the state layout and make_plan.  Every state entry but the num_batches_tracked counters is a source
// of exactly one unit; the units' destination regions are pairwise disjoint, lie inside [0, total) and, with the
// alignment gaps, cover the buffer; offsets are aligned; rows x Kpad is what make_plan reserves; every source
// index of a unit lies inside its tensor, in this file's own words and through pack_unit_fits, the predicate both
// drivers of the pack apply.  Head sets come from the command line (pack_check_sets.h).  Build with a sanitizer:
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined tools/pack_plan_check.cpp -o /tmp/pack_plan_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/pack_plan.h"
#include "pack_check_sets.h"

using namespace sfa;

static long long g_checks = 0, g_bad = 0;
#define EXPECT(cond, ...)                \
  do {                                   \
    ++g_checks;                          \
    if (!(cond)) {                       \
      if (++g_bad <= 20) {               \
        std::printf("BAD %s: ", #cond);  \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

static void check_family(const char* what, const sfa_arch* a, int backbone) {
  const std::vector<Entry> layout = state_layout(a, backbone);
  const Plan p = make_plan(a, backbone);
  const std::vector<PackUnit> units = pack_units(a, backbone);
  const bool deconv = backbone == SFA_BACKBONE_DECONV;
  const int nlev = deconv ? 1 : 3;
  EXPECT(units.size() == (size_t)(17 + 3 + nlev * 2 * a->num_heads), "%s: %zu units", what, units.size());

  // sources: each entry in exactly one unit, every index inside its tensor
  std::vector<int> used(layout.size(), 0);
  auto use = [&](int i, int64_t need, const char* role) {
    EXPECT(i >= 0 && i < (int)layout.size(), "%s: %s index %d", what, role, i);
    if (i < 0 || i >= (int)layout.size()) return;
    ++used[i];
    EXPECT(!is_batches_tracked(layout[i]), "%s: %s reads %s", what, role, layout[i].name.c_str());
    EXPECT(numel(layout[i]) == need, "%s: %s %s has %lld floats, the unit reads %lld", what, role,
           layout[i].name.c_str(), (long long)numel(layout[i]), (long long)need);
  };
  for (const PackUnit& u : units) {
    EXPECT(pack_unit_fits(u, layout), "%s: a unit of %d rows x %d does not fit the drivers", what, u.rows, u.Kpad);
    EXPECT(u.kind == PACK_CONV || u.kind == PACK_DECONV, "%s: kind %d", what, u.kind);
    EXPECT(u.nseg == 1 || u.nseg == 2, "%s: nseg %d", what, u.nseg);
    EXPECT(u.rows > 0 && u.O >= 1 && u.O <= u.rows && u.N > 0, "%s: rows %d O %d N %d", what, u.rows, u.O, u.N);
    EXPECT(u.Kpad > 0 && u.Kpad % 8 == 0 && u.Kpad <= kPackMaxRow, "%s: Kpad %d", what, u.Kpad);
    EXPECT(u.kind == PACK_DECONV ? (u.rows == 4 * u.N && u.nb == u.N) : (u.rows <= u.N && u.nb == u.rows),
           "%s: rows %d N %d nb %d", what, u.rows, u.N, u.nb);
    const int src_rows = u.kind == PACK_DECONV ? u.N : u.O;
    bool any_bn = false;
    for (int s = 0; s < u.nseg; ++s) {
      const PackSeg& sg = u.seg[s];
      use(sg.w, (int64_t)src_rows * sg.I * sg.KH * sg.KW, "weight");
      const bool bn = sg.bn[0] >= 0;
      any_bn = any_bn || bn;
      for (int q = 0; q < 4; ++q) {
        EXPECT((sg.bn[q] >= 0) == bn, "%s: half a BatchNorm", what);
        if (sg.bn[q] >= 0) use(sg.bn[q], src_rows, "BatchNorm");
      }
      EXPECT(sg.I >= 1 && sg.I <= sg.Cpad && sg.k_off >= 0, "%s: I %d Cpad %d k_off %d", what, sg.I, sg.Cpad, sg.k_off);
      if (u.kind == PACK_DECONV) {
        EXPECT(sg.KH == 4 && sg.KW == 4 && 4 * sg.I == u.Kpad, "%s: deconv K", what);
        const size_t n = (size_t)sg.I * u.N * 16;
        size_t worst = 0;
        for (int ph = 0; ph < 4; ++ph)
          for (int k : {0, sg.I - 1, sg.I, 4 * sg.I - 1}) worst = std::max(worst, pack_deconv_src(ph, u.N - 1, k, sg.I, u.N));
        EXPECT(worst < n, "%s: deconv source index %zu of %zu", what, worst, n);
      } else {
        EXPECT(sg.k_off + (sg.KH * sg.KW - 1) * sg.Cpad + sg.I <= u.Kpad, "%s: segment past the row", what);
      }
    }
    if (u.nseg == 2)  // the two segments do not overlap inside the row
      EXPECT(u.seg[0].k_off + u.seg[0].KH * u.seg[0].KW * u.seg[0].Cpad <= u.seg[1].k_off, "%s: segments overlap", what);
    EXPECT((u.bias >= 0) != any_bn, "%s: a unit has a bias or BatchNorm shifts, not both or neither", what);
    if (u.bias >= 0) use(u.bias, u.O, "bias");
  }
  for (size_t i = 0; i < layout.size(); ++i)
    EXPECT(used[i] == (is_batches_tracked(layout[i]) ? 0 : 1), "%s: %s is a source of %d units", what,
           layout[i].name.c_str(), used[i]);

  // destinations: disjoint, inside the buffer, aligned; with the gaps they cover it
  std::vector<std::pair<size_t, size_t>> all;
  for (const PackUnit& u : units) {
    EXPECT(u.w % 16 == 0 && u.b % 4 == 0, "%s: w %zu b %zu", what, u.w, u.b);
    for (size_t o : {u.wx, u.wh}) EXPECT(o == kNoOffset || o % 16 == 0, "%s: term offset %zu", what, o);
    EXPECT(u.winv == kNoOffset || u.winv % 4 == 0, "%s: winv %zu", what, u.winv);
    for (const auto& r : pack_unit_regions(u)) {
      EXPECT(r.first < r.second && r.second <= p.total, "%s: region [%zu, %zu) of %zu", what, r.first, r.second, p.total);
      all.push_back(r);
    }
  }
  std::sort(all.begin(), all.end());
  for (size_t i = 1; i < all.size(); ++i)
    EXPECT(all[i - 1].second <= all[i].first, "%s: regions [%zu, %zu) and [%zu, %zu) overlap", what, all[i - 1].first,
           all[i - 1].second, all[i].first, all[i].second);
  const auto gaps = pack_gaps(units, p.total);
  size_t covered = 0;
  for (const auto& r : all) covered += r.second - r.first;
  for (const auto& g : gaps) {
    covered += g.second - g.first;
    EXPECT(g.second - g.first < 16 && g.second % 16 == 0, "%s: gap [%zu, %zu) is not alignment padding", what, g.first,
           g.second);
  }
  EXPECT(covered == p.total, "%s: regions and gaps cover %zu of %zu floats", what, covered, p.total);
  EXPECT(p.total % 16 == 0, "%s: total %zu", what, p.total);

  // against make_plan: every matrix it reserves is the units' rows x Kpad at its offsets
  size_t ui = 0;
  auto conv = [&](const PConv& c, const char* name) {
    const PackUnit& u = units[ui++];
    EXPECT(u.kind == PACK_CONV && u.rows == c.N && u.N == c.N && u.Kpad == c.Kpad && u.w == c.w && u.b == c.b &&
               u.wx == c.wx && u.wh == c.wh && u.winv == c.winv,
           "%s: %s differs from make_plan", what, name);
  };
  conv(p.stem, "stem");
  for (int li = 0; li < 4; ++li)
    for (int bi = 0; bi < 2; ++bi)
      for (int ci = 0; ci < 2; ++ci) {
        EXPECT(units[ui].nseg == (ci == 1 && bi == 0 && li > 0 ? 2 : 1), "%s: layer%d.%d conv%d segments", what, li + 1, bi,
               ci + 1);
        conv(p.blk[li][bi][ci], "body conv");
      }
  for (int i = 0; i < 3; ++i) {
    if (!deconv) {
      conv(p.fpn[i], "fpn conv");
      continue;
    }
    const PackUnit& u = units[ui++];
    const PDeconv& d = p.dec[i];
    EXPECT(u.kind == PACK_DECONV && u.rows == 4 * d.N && u.N == d.N && u.Kpad == d.K && u.seg[0].I == d.C && u.w == d.w &&
               u.b == d.b && u.wx == kNoOffset && u.wh == d.wh && u.winv == d.winv,
           "%s: deconv %d differs from make_plan", what, i);
  }
  for (int f = 0; f < nlev; ++f) {
    const PHeads& h = p.heads[f];
    long long rows = 0;
    for (int j = 0; j < a->num_heads; ++j) {
      const PackUnit& u = units[ui++];
      const PackUnit& w1 = units[ui++];
      EXPECT(u.rows == 64 && u.N == h.N && u.Kpad == h.K && u.w == h.w3 + (size_t)rows * h.K && u.b == h.b3 + rows &&
                 u.wx == h.wx + (size_t)rows * h.K / 2 && u.wh == h.wh + (size_t)rows * h.K / 2 && u.winv == h.winv + rows,
             "%s: level %d head %d differs from make_plan", what, f, j);
      EXPECT(w1.rows == 4 && w1.O == a->head_channels[j] && w1.Kpad == 64 && w1.w == h.w1 + (size_t)j * 256 &&
                 w1.b == h.b1 + (size_t)j * 4 && w1.wx == kNoOffset && w1.wh == kNoOffset && w1.winv == kNoOffset,
             "%s: level %d head %d w1 differs from make_plan", what, f, j);
      rows += u.rows;
    }
    EXPECT(rows == h.N, "%s: level %d has %lld of %d rows", what, f, rows, h.N);
  }
  EXPECT(ui == units.size(), "%s: %zu units walked of %zu", what, ui, units.size());
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
  std::printf("%zu head sets, %lld checks, %lld bad\n", sets.size(), g_checks, g_bad);
  return g_bad ? 1 : 0;
}
