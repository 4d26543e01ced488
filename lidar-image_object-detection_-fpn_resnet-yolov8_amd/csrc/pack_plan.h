// The packed-weight plan: the reference state_dict layout of both families, the offsets of every packed
// matrix (make_plan) and the flat list of pack units, the one description of the pack that sfa_pack_weights
// (pack_host.h) and its device form (pack_kernel.h) both walk. Plain C++ (no HIP include, g++ builds it):
// tools/pack_plan_check.cpp walks it on the CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sfa_hip.h"
#include "host_math.h"

namespace sfa {

// The descriptor checks of every layout / pack / create entry (pack.hip); only declared here.
int check_arch(const sfa_arch* a, int backbone = SFA_BACKBONE_KFPN);
int check_arch_ex(const sfa_arch_ex* x);

struct Entry {
  std::string name;
  std::vector<int64_t> shape;
};

inline int64_t numel(const Entry& e) {
  int64_t n = 1;
  for (auto s : e.shape) n *= s;
  return n;
}

static const int kFpnC[3] = {256, 128, 64};

inline std::vector<int> sorted_heads(const sfa_arch* a) {
  std::vector<int> idx(a->num_heads);
  for (int j = 0; j < a->num_heads; ++j) idx[j] = j;
  std::sort(idx.begin(), idx.end(), [&](int x, int y) {
    return std::string(a->head_names[x]) < std::string(a->head_names[y]);
  });
  return idx;
}

// nn.Module registration order of PoseResNet (fpn_resnet.py:114-151, 42-53; resnet.py:117-158 for
// the deconv family: deconv_layers.{0,3,6} ConvTranspose2d (Cin, 256, 4, 4), .{1,4,7} BatchNorm, then
// the heads under their plain names).
inline std::vector<Entry> state_layout(const sfa_arch* a, int backbone = SFA_BACKBONE_KFPN) {
  std::vector<Entry> v;
  auto bn = [&](const std::string& p, int64_t c) {
    v.push_back({p + ".weight", {c}});
    v.push_back({p + ".bias", {c}});
    v.push_back({p + ".running_mean", {c}});
    v.push_back({p + ".running_var", {c}});
    v.push_back({p + ".num_batches_tracked", {}});
  };
  v.push_back({"conv1.weight", {64, 3, 7, 7}});
  bn("bn1", 64);
  int inplanes = 64;
  for (int li = 1; li <= 4; ++li) {
    const int planes = 64 << (li - 1);
    for (int bi = 0; bi < 2; ++bi) {
      const std::string p = "layer" + std::to_string(li) + "." + std::to_string(bi);
      const int cin = bi == 0 ? inplanes : planes;
      v.push_back({p + ".conv1.weight", {planes, cin, 3, 3}});
      bn(p + ".bn1", planes);
      v.push_back({p + ".conv2.weight", {planes, planes, 3, 3}});
      bn(p + ".bn2", planes);
      if (bi == 0 && (li > 1)) {
        v.push_back({p + ".downsample.0.weight", {planes, inplanes, 1, 1}});
        bn(p + ".downsample.1", planes);
      }
    }
    inplanes = planes;
  }
  const auto order = sorted_heads(a);
  if (backbone == SFA_BACKBONE_DECONV) {
    for (int i = 0; i < 3; ++i) {
      v.push_back({"deconv_layers." + std::to_string(3 * i) + ".weight", {i == 0 ? 512 : 256, 256, 4, 4}});
      bn("deconv_layers." + std::to_string(3 * i + 1), 256);
    }
    for (int j : order) {
      const std::string p = a->head_names[j];
      v.push_back({p + ".0.weight", {a->head_conv, 256, 3, 3}});
      v.push_back({p + ".0.bias", {a->head_conv}});
      v.push_back({p + ".2.weight", {a->head_channels[j], a->head_conv, 1, 1}});
      v.push_back({p + ".2.bias", {a->head_channels[j]}});
    }
    return v;
  }
  const int up_out[3] = {256, 128, 64}, up_in[3] = {768, 384, 192};
  for (int i = 0; i < 3; ++i) {
    const std::string p = "conv_up_level" + std::to_string(i + 1);
    v.push_back({p + ".weight", {up_out[i], up_in[i], 1, 1}});
    v.push_back({p + ".bias", {up_out[i]}});
  }
  for (int f = 0; f < 3; ++f)
    for (int j : order) {
      const std::string p = "fpn" + std::to_string(f) + "_" + a->head_names[j];
      v.push_back({p + ".0.weight", {a->head_conv, kFpnC[f], 3, 3}});
      v.push_back({p + ".0.bias", {a->head_conv}});
      v.push_back({p + ".2.weight", {a->head_channels[j], a->head_conv, 1, 1}});
      v.push_back({p + ".2.bias", {a->head_channels[j]}});
    }
  return v;
}

inline bool is_batches_tracked(const Entry& e) { return e.name.find("num_batches_tracked") != std::string::npos; }

// ----------------------------------------------------------- packed layout
// Offsets in floats into the packed buffer.  wx: the same weights split into three
// bf16 terms [3][N][Kpad] for the bf16x6 kernels (conv_x6_kernel.h); wh / winv: the
// fp16x3 form, W[n][k] * 2^e[n] as two fp16 terms [2][N][Kpad] and winv[n] = 2^-e[n].
struct PConv {
  size_t w, b, wx, wh, winv;
  int N, K, Kpad;
};
struct PHeads {
  size_t w3, b3, w1, b1, wx, wh, winv;
  int N, K;
};
// One transposed conv (deconv_h3_kernel.h): w = the four phase matrices [4][N][K] f32, K = 4 C in
// (dy, dx, c) order, BN scale folded in; b = the BN shift [N]; wh = [4][2][N][K] fp16 terms and
// winv = [4][N], split per phase and row.
struct PDeconv {
  size_t w, b, wh, winv;
  int N, C, K;
};
struct Plan {
  int backbone;
  PConv stem;
  PConv blk[4][2][2];  // [layer][block][conv1, conv2(+downsample)]
  PConv fpn[3];        // KFPN
  PDeconv dec[3];      // deconv family
  PHeads heads[3];     // KFPN: per level; deconv family: heads[0] alone (256 channels in)
  size_t total;
};

inline Plan make_plan(const sfa_arch* a, int backbone = SFA_BACKBONE_KFPN) {
  Plan p;
  memset(&p, 0, sizeof p);
  p.backbone = backbone;
  size_t cur = 0;
  auto take = [&](size_t n) {
    const size_t o = cur;
    cur = align_up(cur + n, 16);
    return o;
  };
  auto conv = [&](int N, int K) {
    PConv c;
    c.N = N;
    c.K = K;
    c.Kpad = (int)align_up(K, 16);
    c.w = take((size_t)N * c.Kpad);
    c.b = take(N);
    c.wx = take(((size_t)3 * N * c.Kpad + 1) / 2);
    c.wh = take((size_t)N * c.Kpad);
    c.winv = take(N);
    return c;
  };
  p.stem = conv(64, 49 * 4);
  int inplanes = 64;
  for (int li = 0; li < 4; ++li) {
    const int planes = 64 << li;
    for (int bi = 0; bi < 2; ++bi) {
      const int cin = bi == 0 ? inplanes : planes;
      const bool ds = bi == 0 && li > 0;
      p.blk[li][bi][0] = conv(planes, 9 * cin);
      p.blk[li][bi][1] = conv(planes, 9 * planes + (ds ? inplanes : 0));
    }
    inplanes = planes;
  }
  const bool deconv = backbone == SFA_BACKBONE_DECONV;
  if (deconv) {
    for (int i = 0; i < 3; ++i) {
      PDeconv& d = p.dec[i];
      d.N = 256;
      d.C = i == 0 ? 512 : 256;
      d.K = 4 * d.C;
      d.w = take((size_t)4 * d.N * d.K);
      d.b = take(d.N);
      d.wh = take((size_t)4 * d.N * d.K);
      d.winv = take((size_t)4 * d.N);
    }
  } else {
    p.fpn[0] = conv(256, 768);
    p.fpn[1] = conv(128, 384);
    p.fpn[2] = conv(64, 192);
  }
  for (int f = 0; f < (deconv ? 1 : 3); ++f) {
    PHeads& h = p.heads[f];
    h.N = a->num_heads * a->head_conv;
    h.K = 9 * kFpnC[f];
    h.w3 = take((size_t)h.N * h.K);
    h.b3 = take(h.N);
    h.w1 = take((size_t)a->num_heads * 4 * 64);
    h.b1 = take((size_t)a->num_heads * 4);
    h.wx = take(((size_t)3 * h.N * h.K + 1) / 2);
    h.wh = take((size_t)h.N * h.K);
    h.winv = take(h.N);
  }
  p.total = cur;
  return p;
}

// ----------------------------------------------------------- pack units
// One unit = one packed matrix (or the rows one state tensor gives to a shared one): `rows` rows of `Kpad`
// floats gathered from one or two source segments, then split into terms.  All sources are indices into
// state_layout (-1: none); all destinations are float offsets into the packed buffer (kNoOffset: none).
constexpr size_t kNoOffset = ~(size_t)0;
constexpr int kPackMaxRow = 4864;  // the longest packed row (layer4.0 conv2 + downsample): the pack kernel's LDS row

enum PackKind {
  PACK_CONV = 0,    // OIHW source, row o: W[o][k_off + (kh KW + kw) Cpad + c] = w[o][c][kh][kw] * scale[o]
  PACK_DECONV = 1,  // (Cin, Cout, 4, 4) source, rows = 4 phases x N: row ph N + n, see pack_deconv_src
};

struct PackSeg {
  int w;      // the weight
  int bn[4];  // BatchNorm weight, bias, running_mean, running_var folded into it (all -1: scale 1, shift 0)
  int I, KH, KW, Cpad, k_off;
};

struct PackUnit {
  int kind;
  int O;     // rows the source has; rows [O, rows) of the unit are zero (w1 / b1 of a narrower head)
  int rows;  // packed rows of this unit
  int N;     // rows of one term plane of the matrix the unit belongs to (>= rows for PACK_CONV)
  int Kpad;  // packed row length; the terms of row r start (r / N) * 2 * N * Kpad + (r % N) * Kpad 2-byte
             // values after the unit's wx / wh, term t another t * N * Kpad after that
  int nseg;
  PackSeg seg[2];
  int bias;  // a plain bias copied to b (-1: b = the sum of the segments' BatchNorm shifts)
  int nb;    // entries of b this unit writes (PACK_DECONV: N, by phase 0's rows; otherwise rows)
  size_t w, b, wx, wh, winv;
};

// Source index of element k = (2 dy + dx) C + c of row n of phase ph = 2 py + px of a transposed conv
// (Cin = C, Cout = N, 4 x 4): w[c][n][3 - py - 2 dy][3 - px - 2 dx] (deconv_h3_kernel.h).  constexpr: the pack
// kernel calls it too.
constexpr size_t pack_deconv_src(int ph, int n, int k, int C, int N) {
  const int py = ph >> 1, px = ph & 1, tap = k / C, c = k % C, dy = tap >> 1, dx = tap & 1;
  return (((size_t)c * N + n) * 4 + (3 - py - 2 * dy)) * 4 + (3 - px - 2 * dx);
}

inline std::vector<PackUnit> pack_units(const sfa_arch* a, int backbone = SFA_BACKBONE_KFPN) {
  const std::vector<Entry> layout = state_layout(a, backbone);
  const Plan p = make_plan(a, backbone);
  auto idx = [&](const std::string& name) {
    for (size_t i = 0; i < layout.size(); ++i)
      if (layout[i].name == name) return (int)i;
    return -1;
  };
  auto seg = [&](const std::string& w, const std::string& bn, int I, int KH, int KW, int Cpad, int k_off) {
    PackSeg s{idx(w), {-1, -1, -1, -1}, I, KH, KW, Cpad, k_off};
    if (!bn.empty()) {
      const char* leaf[4] = {".weight", ".bias", ".running_mean", ".running_var"};
      for (int i = 0; i < 4; ++i) s.bn[i] = idx(bn + leaf[i]);
    }
    return s;
  };
  auto conv = [&](const PConv& c, const PackSeg& s0) {
    PackUnit u{};
    u.kind = PACK_CONV;
    u.O = u.rows = u.N = u.nb = c.N;
    u.Kpad = c.Kpad;
    u.nseg = 1;
    u.seg[0] = s0;
    u.bias = -1;
    u.w = c.w, u.b = c.b, u.wx = c.wx, u.wh = c.wh, u.winv = c.winv;
    return u;
  };
  std::vector<PackUnit> v;
  // stem: conv1 + bn1, input channels padded 3 -> 4
  v.push_back(conv(p.stem, seg("conv1.weight", "bn1", 3, 7, 7, 4, 0)));
  int inplanes = 64;
  for (int li = 0; li < 4; ++li) {
    const int planes = 64 << li;
    for (int bi = 0; bi < 2; ++bi) {
      const std::string pre = "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      const int cin = bi == 0 ? inplanes : planes;
      v.push_back(conv(p.blk[li][bi][0], seg(pre + ".conv1.weight", pre + ".bn1", cin, 3, 3, cin, 0)));
      PackUnit u = conv(p.blk[li][bi][1], seg(pre + ".conv2.weight", pre + ".bn2", planes, 3, 3, planes, 0));
      if (bi == 0 && li > 0) {  // the downsample: a second segment of the same rows, b = sh + sh2
        u.nseg = 2;
        u.seg[1] = seg(pre + ".downsample.0.weight", pre + ".downsample.1", inplanes, 1, 1, inplanes, 9 * planes);
      }
      v.push_back(u);
    }
    inplanes = planes;
  }
  const bool deconv = backbone == SFA_BACKBONE_DECONV;
  for (int i = 0; deconv && i < 3; ++i) {
    const PDeconv& d = p.dec[i];
    PackUnit u{};
    u.kind = PACK_DECONV;
    u.O = u.rows = 4 * d.N;
    u.N = u.nb = d.N;
    u.Kpad = d.K;
    u.nseg = 1;
    u.seg[0] = seg("deconv_layers." + std::to_string(3 * i) + ".weight", "deconv_layers." + std::to_string(3 * i + 1),
                   d.C, 4, 4, d.C, 0);
    u.bias = -1;
    u.w = d.w, u.b = d.b, u.wx = kNoOffset, u.wh = d.wh, u.winv = d.winv;
    v.push_back(u);
  }
  const int up_in[3] = {768, 384, 192};
  for (int i = 0; !deconv && i < 3; ++i) {
    const std::string pre = "conv_up_level" + std::to_string(i + 1);
    PackUnit u = conv(p.fpn[i], seg(pre + ".weight", "", up_in[i], 1, 1, up_in[i], 0));
    u.bias = idx(pre + ".bias");
    v.push_back(u);
  }
  for (int f = 0; f < (deconv ? 1 : 3); ++f) {
    const PHeads& hp = p.heads[f];
    for (int j = 0; j < a->num_heads; ++j) {
      const std::string pre =
          deconv ? std::string(a->head_names[j]) : "fpn" + std::to_string(f) + "_" + a->head_names[j];
      PackUnit u{};  // the head's 64 rows of the level's 3x3 matrix
      u.kind = PACK_CONV;
      u.O = u.rows = u.nb = 64;
      u.N = hp.N;
      u.Kpad = hp.K;
      u.nseg = 1;
      u.seg[0] = seg(pre + ".0.weight", "", kFpnC[f], 3, 3, kFpnC[f], 0);
      u.bias = idx(pre + ".0.bias");
      const size_t r0 = (size_t)j * 64;
      u.w = hp.w3 + r0 * hp.K, u.b = hp.b3 + r0, u.wx = hp.wx + r0 * hp.K / 2, u.wh = hp.wh + r0 * hp.K / 2;
      u.winv = hp.winv + r0;
      v.push_back(u);
      PackUnit w1{};  // its 1x1 conv: four rows, zero from head_channels[j] on
      w1.kind = PACK_CONV;
      w1.O = a->head_channels[j];
      w1.rows = w1.N = w1.nb = 4;
      w1.Kpad = 64;
      w1.nseg = 1;
      w1.seg[0] = seg(pre + ".2.weight", "", 64, 1, 1, 64, 0);
      w1.bias = idx(pre + ".2.bias");
      w1.w = hp.w1 + (size_t)j * 4 * 64, w1.b = hp.b1 + (size_t)j * 4;
      w1.wx = w1.wh = w1.winv = kNoOffset;
      v.push_back(w1);
    }
  }
  return v;
}

// Whether both drivers of the pack (pack_host.h, pack_kernel.h) can walk the unit: a row of 8-element steps that
// fits the kernel's LDS row, every segment inside the row, and every source index inside the tensor `layout`
// describes (the weight rows x I x KH x KW, a whole BatchNorm quadruple or none, the bias).
inline bool pack_unit_fits(const PackUnit& u, const std::vector<Entry>& layout) {
  auto holds = [&](int i, int64_t n) { return i >= 0 && i < (int)layout.size() && numel(layout[i]) == n; };
  const bool deconv = u.kind == PACK_DECONV;
  bool ok = (deconv || u.kind == PACK_CONV) && u.Kpad > 0 && u.Kpad % 8 == 0 && u.Kpad <= kPackMaxRow && u.N > 0 &&
            u.O >= 1 && u.O <= u.rows && (deconv ? u.rows == 4 * u.N : u.rows <= u.N) && (u.nseg == 1 || u.nseg == 2) &&
            (u.bias >= 0 || u.seg[0].bn[0] >= 0);
  const int src_rows = deconv ? u.N : u.O;
  for (int s = 0; ok && s < u.nseg; ++s) {
    const PackSeg& sg = u.seg[s];
    ok = sg.I >= 1 && sg.I <= sg.Cpad && sg.KH >= 1 && sg.KW >= 1 && sg.k_off >= 0 && (!deconv || sg.KH * sg.KW == 16);
    const int last = deconv ? 4 * sg.I : sg.k_off + (sg.KH * sg.KW - 1) * sg.Cpad + sg.I;
    ok = ok && last <= u.Kpad && holds(sg.w, (int64_t)src_rows * sg.I * sg.KH * sg.KW);
    for (int q = 0; q < 4; ++q) ok = ok && (sg.bn[q] < 0 ? sg.bn[0] < 0 : holds(sg.bn[q], src_rows));
  }
  return ok && (u.bias < 0 || holds(u.bias, u.O));
}

// The destination regions of a unit, [first, second) in floats.
inline std::vector<std::pair<size_t, size_t>> pack_unit_regions(const PackUnit& u) {
  std::vector<std::pair<size_t, size_t>> r;
  const size_t row = (size_t)u.rows * u.Kpad, plane = (size_t)u.N * u.Kpad;
  r.push_back({u.w, u.w + row});
  r.push_back({u.b, u.b + u.nb});
  const int phases = (u.rows + u.N - 1) / u.N;
  const size_t per = std::min(row, plane);  // 2-byte values of one term of one phase
  if (u.wx != kNoOffset)
    for (int t = 0; t < 3; ++t) r.push_back({u.wx + t * plane / 2, u.wx + (t * plane + per) / 2});
  if (u.wh != kNoOffset)
    for (int ph = 0; ph < phases; ++ph)
      for (int t = 0; t < 2; ++t)
        r.push_back({u.wh + (ph * 2 + t) * plane / 2, u.wh + ((ph * 2 + t) * plane + per) / 2});
  if (u.winv != kNoOffset) r.push_back({u.winv, u.winv + u.rows});
  return r;
}

// The floats of [0, total) no unit writes: the alignment gaps, which the pack zeroes.
inline std::vector<std::pair<size_t, size_t>> pack_gaps(const std::vector<PackUnit>& units, size_t total) {
  std::vector<std::pair<size_t, size_t>> all, gaps;
  for (const PackUnit& u : units)
    for (const auto& r : pack_unit_regions(u)) all.push_back(r);
  std::sort(all.begin(), all.end());
  size_t cur = 0;
  for (const auto& r : all) {
    if (r.first > cur) gaps.push_back({cur, r.first});
    cur = std::max(cur, r.second);
  }
  if (cur < total) gaps.push_back({cur, total});
  return gaps;
}

}  // namespace sfa
