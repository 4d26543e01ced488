// Stand-alone check of the decode geometry (csrc/decode_plan.h), host only: every map of up to
// kTileMaxHW cells gets a tile plan within the tile kernel's per-workgroup limits whose tiles cover
// the map exactly once, the workspace layout is ordered and aligned, and the band and class forms'
// lists fit the size sfa_decode_workspace_size reserves.  Build with a sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/decode_plan_check.cpp -o /tmp/decode_plan_check
#include <cstdio>
#include <vector>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/decode_plan.h"

using namespace sfa;

static int check(int H, int W, bool cover) {
  int R, TC, NY, NX;
  if (!tile_plan(H, W, &R, &TC, &NY, &NX)) return std::printf("no plan for %d x %d\n", H, W), 1;
  const bool ok = R >= 1 && TC >= 1 && (R + 2) * (TC + 2) <= kBandMaxTile &&
                  (R + 2) * (TC + 2) <= kBandMaxLoads * kBandThreads && R * TC <= kBandMaxIPT * kBandThreads &&
                  (NY - 1) * R < H && NY * R >= H && (NX - 1) * TC < W && NX * TC >= W;
  if (!ok) return std::printf("bad plan for %d x %d: R %d TC %d NY %d NX %d\n", H, W, R, TC, NY, NX), 1;
  if (cover) {
    std::vector<unsigned char> seen((size_t)H * W, 0);
    for (int t = 0; t < NY * NX; ++t) {
      const int ty = t / NX, x0 = (t - ty * NX) * TC, y0 = ty * R;
      const int tw = TC < W - x0 ? TC : W - x0, y1 = H < y0 + R ? H : y0 + R;
      int last = -1;  // a tile's pixels in the kernel's order: rows of the tile, left to right
      for (int y = y0; y < y1; ++y)
        for (int idx = y * W + x0; idx < y * W + x0 + tw; ++idx) {
          if (idx <= last || seen[idx]++) return std::printf("order / overlap at %d x %d\n", H, W), 1;
          last = idx;
        }
    }
    for (unsigned char s : seen)
      if (s != 1) return std::printf("uncovered cell at %d x %d\n", H, W), 1;
  }
  const TiledLayout l = tiled_layout(64, 16, NY * NX, kDecMaxK);
  if (!(l.tile_idx % 256 == 0 && l.class_key % 256 == 0 && l.class_idx % 256 == 0 && l.tile_idx < l.class_key &&
        l.class_key < l.class_idx && l.class_idx < l.total))
    return std::printf("bad layout at %d x %d\n", H, W), 1;
  return 0;
}

// Band / class forms (maps of up to kDecMaxHW cells): whatever band_plan picks, the lists lie inside
// list_workspace_bytes, the size sfa_decode_workspace_size returns, with the index part 256-B aligned.
static int check_lists(int H, int W) {
  if ((long long)H * W > kDecMaxHW) return 0;
  int bad = 0;
  for (int C : {1, 3, 16})
    for (int K : {1, 40, 50, 256}) {
      if (K > H * W) continue;
      int S, R;
      band_plan(C, H, W, K, &S, &R);
      if (S < 0 || S > kBandMaxS || (S > 0 && (R < 1 || S * R < H || (S - 1) * R >= H))) {
        bad += std::printf("bad band plan for %d x %d x %d K %d: S %d R %d\n", C, H, W, K, S, R) > 0;
        continue;
      }
      for (int B : {1, 3, 64}) {
        const ListLayout l = list_layout(B, C, S > 0 ? S : 1, K);
        const size_t n = (size_t)B * C * (S > 0 ? S : 1) * K;
        if (!(l.idx % 256 == 0 && l.idx >= n * sizeof(unsigned) && l.idx + n * sizeof(int) <= l.total &&
              l.total <= list_workspace_bytes(B, C, K)))
          bad += std::printf("lists of %d x %d x %d x %d K %d outside the workspace\n", B, C, H, W, K) > 0;
      }
    }
  return bad;
}

int main() {
  int bad = 0, n = 0, max_nt = 0;
  for (int H = 1; H <= kTileMaxHW; H = H < 600 ? H + 1 : H * 2 + 1)
    for (int W = 1; (long long)H * W <= kTileMaxHW; W = W < 600 ? W + 1 : W + W / 3 + 1, ++n) {
      bad += check(H, W, (H * W) % 7 == 0);
      if ((H + W) % 13 == 0 || H * W <= 64) bad += check_lists(H, W);
      int R, TC, NY, NX;
      tile_plan(H, W, &R, &TC, &NY, &NX);
      if (NY * NX > max_nt) max_nt = NY * NX;
    }
  const int edge[][2] = {{1, kTileMaxHW}, {kTileMaxHW, 1}, {512, 512}, {200, 200}, {193, 192}, {3, 16384}, {16384, 3},
                         {1, 40000}, {2, 131072}, {255, 1025}};
  for (auto& e : edge) bad += check(e[0], e[1], true);
  const int small[][2] = {{152, 152}, {37, 29}, {3, 4100}, {192, 192}, {1, kDecMaxHW}, {kDecMaxHW, 1}, {96, 96}, {8, 4608}};
  for (auto& e : small) bad += check_lists(e[0], e[1]);
  int R, TC, NY, NX;
  bad += tile_plan(513, 512, &R, &TC, &NY, &NX) || tile_plan(0, 5, &R, &TC, &NY, &NX) ||
         tile_plan(65536, 65536, &R, &TC, &NY, &NX);
  int S, Rb;
  band_plan(3, 152, 152, 50, &S, &Rb);
  bad += !(S == 8 && Rb == 19);
  band_plan(3, 37, 29, 50, &S, &Rb);  // 8 bands of 5 rows: 3 * 8 * 50 candidates, 7 x 31 tile
  bad += !(S == 8 && Rb == 5);
  band_plan(3, 3, 4100, 40, &S, &Rb);  // a 4102-float row with its halo fills more than half a tile: class form
  bad += S != 0;
  bad += list_workspace_bytes(2, 3, 50) != 2 * 19200;  // 2 * 3 * 50 * 16 words = 19,200 B, keys then indices
  std::printf("%d shapes, most tiles per class map %d, %d bad\n", n, max_nt, bad);
  return bad != 0;
}
