// Decode geometry: the limits of the top-K kernels (decode.hip) and the host functions that cut a
// class map into band or tile workgroups.  Plain C++ (no HIP), so the plans can be compiled and
// checked on their own (tools/decode_plan_check.cpp).
#pragma once

#include <cstddef>

namespace sfa {

constexpr int kDecThreads = 1024;
constexpr int kDecMaxHW = 36864;  // 144 KiB of LDS: the largest map the whole-map / band kernels take
constexpr int kDecMaxK = 256;

constexpr int kBandThreads = 512;
constexpr int kBandWaves = kBandThreads / 64;
constexpr int kBandMaxTile = 8192;   // LDS floats of a band tile ((R + 2) x (W + 2), -inf border)
constexpr int kBandMaxIPT = 8;       // band pixels per thread
constexpr int kBandMaxLoads = 16;    // staged tile floats per thread
constexpr int kMergeMax = 4096;      // C * S * K candidates ranked per frame

constexpr int kTileMaxHW = 1 << 18;  // 512 x 512: the largest map of the tiled form (any aspect)
constexpr int kTileMaxCols = 1024;   // a wider row is cut into column tiles

// Band geometry: S bands of R rows (8 preferred: 384 workgroups at B = 16, C = 3) with
// C * S * K <= kMergeMax, (R + 2) * (W + 2) <= kBandMaxTile and ceil(R * W / 512) <= kBandMaxIPT;
// S = 0 when no band split fits (one block per class).
inline void band_plan(int C, int H, int W, int K, int* S_out, int* R_out) {
  *S_out = 0;
  *R_out = H;
  static const int order[] = {8, 9, 10, 11, 12, 13, 14, 15, 16, 7, 6, 5, 4, 3, 2, 1};
  for (int S : order) {
    if (S > H) continue;
    const int R = (H + S - 1) / S;
    const int S_eff = (H + R - 1) / R;
    if (C * S_eff * K > kMergeMax) continue;
    if ((R + 2) * (W + 2) > kBandMaxTile || (R + 2) * (W + 2) > kBandMaxLoads * kBandThreads) continue;
    if ((R * W + kBandThreads - 1) / kBandThreads > kBandMaxIPT) continue;
    *S_out = S_eff;
    *R_out = R;
    return;
  }
}

// Tile geometry for maps above kDecMaxHW: NY x NX tiles of R rows x TC columns (the last row /
// column of tiles may be shorter), each within the band kernel's per-workgroup limits:
// (R + 2) * (TC + 2) <= kBandMaxTile and kBandMaxLoads * kBandThreads (tile + 1-cell halo) and
// R * TC <= kBandMaxIPT * kBandThreads.  Rows are cut evenly (R = ceil(H / NY)); a row wider than
// kTileMaxCols is cut into NX even column ranges.  false when the map is outside 1 <= H*W <= kTileMaxHW.
inline bool tile_plan(int H, int W, int* R_out, int* TC_out, int* NY_out, int* NX_out) {
  if (H < 1 || W < 1 || (long long)H * W > kTileMaxHW) return false;
  const int nx0 = (W + kTileMaxCols - 1) / kTileMaxCols;
  const int tc = (W + nx0 - 1) / nx0;  // <= kTileMaxCols
  const int lds = kBandMaxTile < kBandMaxLoads * kBandThreads ? kBandMaxTile : kBandMaxLoads * kBandThreads;
  int r = kBandMaxIPT * kBandThreads / tc;         // >= 4
  if (lds / (tc + 2) - 2 < r) r = lds / (tc + 2) - 2;  // >= 5 at tc = 1024
  if (r > H) r = H;
  const int ny = (H + r - 1) / r;
  *R_out = (H + ny - 1) / ny;
  *TC_out = tc;
  *NY_out = (H + *R_out - 1) / *R_out;
  *NX_out = (W + tc - 1) / tc;
  return true;
}

inline size_t plan_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Workspace of the band and class forms: `lists` sorted K-lists per (frame, class) (the S bands, or
// 1), keys at 0, then indices; both parts 256-B aligned.
struct ListLayout {
  size_t idx, total;  // byte offsets
};
inline ListLayout list_layout(int B, int C, int lists, int K) {
  const size_t n = (size_t)B * C * lists * K;
  ListLayout l;
  l.idx = plan_align_up(n * sizeof(unsigned), 256);
  l.total = l.idx + plan_align_up(n * sizeof(int), 256);
  return l;
}
// band_plan gives S <= 16 (its largest candidate), so room for 16 lists per class holds either form:
// the entries check the workspace against this size once, and no form needs a check of its own.
constexpr int kBandMaxS = 16;
inline size_t list_workspace_bytes(int B, int C, int K) { return list_layout(B, C, kBandMaxS, K).total; }

// Workspace of the tiled form: NT = NY * NX sorted K-lists per (frame, class) (keys, then
// indices), then one merged K-list per (frame, class) (keys, then indices); every part 256-B aligned.
struct TiledLayout {
  size_t tile_idx, class_key, class_idx, total;  // byte offsets (tile keys at 0)
};
inline TiledLayout tiled_layout(int B, int C, int NT, int K) {
  const size_t nt = (size_t)B * C * NT * K, nc = (size_t)B * C * K;
  TiledLayout l;
  l.tile_idx = plan_align_up(nt * sizeof(unsigned), 256);
  l.class_key = l.tile_idx + plan_align_up(nt * sizeof(int), 256);
  l.class_idx = l.class_key + plan_align_up(nc * sizeof(unsigned), 256);
  l.total = l.class_idx + plan_align_up(nc * sizeof(int), 256);
  return l;
}

}  // namespace sfa
