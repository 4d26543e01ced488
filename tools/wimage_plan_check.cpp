// Stand-alone host check of the pre-tiled weight images' index function and plan (csrc/conv_wimage.h):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/wimage_plan_check.cpp -o /tmp/wimage_plan_check
//   /tmp/wimage_plan_check                 # the self-check: "wimage_plan_check: N checks, 0 bad"
//   /tmp/wimage_plan_check dump N K wstride wk0 BN terms cmaj_tiles C
//                                          # one line "term n k" per (nt, kt, e, lane), in image order
// The self-check walks one geometry per kernel family that stages W by LDS-DMA (the heads' 256 x 320
// chunk-major tile, the 128 x 128 and 128 x 64 tiles tap-major and chunk-major, a K-slice of a wider conv,
// a tile whose pieces do not divide among 4 or 8 waves) and checks, against a restatement that starts from
// the LDS side (per term, rows of 64 B, source quad q of row R at quad q ^ swzB(R)):
//  * the image is dense: offsets 0, 16, .. bytes - 16, each once;
//  * every source quad (term, row, 8 K columns) of the slice is read exactly once, inside the terms array;
//  * image byte (kt slot, term, R, quad position p) holds source quad p ^ swzB(R) of row n0 + R at the
//    K-tile's columns, so a lane that reads quad (g ^ swzB(c16)) of row c16 of a column block gets
//    k = 8 g .. 8 g + 7: the fragment the MFMAs take;
//  * pieces e = wave + NW j, j < ceil(pieces / NW), e < pieces cover each piece once (also when pieces % NW != 0);
//  * the model plan's regions are 256-B aligned, disjoint and inside the total; bad geometries are refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/conv_wimage.h"

using namespace sfa;

static long long g_checks = 0, g_bad = 0;
#define CHECK(c, ...)                \
  do {                               \
    ++g_checks;                      \
    if (!(c)) {                      \
      ++g_bad;                       \
      if (g_bad < 20) {              \
        std::printf("BAD %s: ", #c); \
        std::printf(__VA_ARGS__);    \
        std::printf("\n");           \
      }                              \
    }                                \
  } while (0)

// the kernels' swizzle, written from the comment's words: bits 2..3 of the row, xor'ed with whether
// (row % 16) + 4 has bit 3 set
static int swz_restated(int R) {
  const int hi = (R / 4) % 4;
  const int r16 = R % 16;
  const int bit = (r16 + 4) / 8 % 2;
  return hi ^ bit;
}

static void check_geom(const WImageGeom& g, const char* name) {
  CHECK(wimage_check(g) == nullptr, "%s: %s", name, wimage_check(g));
  if (wimage_check(g)) return;
  const int ntile = g.N / g.BN, kt_n = wimage_ktiles(g), pieces = wimage_pieces(g);
  const size_t bytes = wimage_bytes(g);
  CHECK(bytes == (size_t)g.terms * g.N * g.K * 2, "%s: image %zu bytes, slice %zu", name, bytes,
        (size_t)g.terms * g.N * g.K * 2);
  std::vector<unsigned char> seen_img(bytes / 16, 0);
  // one flag per source quad of the terms array [terms][N][wstride / 8]
  std::vector<unsigned char> seen_src((size_t)g.terms * g.N * (g.wstride / 8), 0);
  // each K column block of 32 of the slice is some K-tile's: tiles are a permutation of the slice
  std::vector<int> kcols(kt_n, 0);
  for (int kt = 0; kt < kt_n; ++kt) {
    const int kc = wimage_kcol(g, kt);
    CHECK(kc >= 0 && kc % 32 == 0 && kc / 32 < kt_n, "%s: kcol(%d) = %d", name, kt, kc);
    if (kc >= 0 && kc % 32 == 0 && kc / 32 < kt_n) ++kcols[kc / 32];
  }
  for (int i = 0; i < kt_n; ++i) CHECK(kcols[i] == 1, "%s: K block %d in %d tiles", name, i, kcols[i]);
  for (int nt = 0; nt < ntile; ++nt)
    for (int kt = 0; kt < kt_n; ++kt)
      for (int e = 0; e < pieces; ++e)
        for (int l = 0; l < 64; ++l) {
          int term, n, k;
          const size_t src = wimage_source(g, nt, kt, e, l, &term, &n, &k);
          const size_t off = wimage_offset(g, nt, kt, e, l);
          CHECK(off % 16 == 0 && off + 16 <= bytes, "%s: offset %zu of %zu", name, off, bytes);
          if (off + 16 <= bytes) {
            CHECK(!seen_img[off / 16], "%s: image offset %zu twice", name, off);
            seen_img[off / 16] = 1;
          }
          CHECK(term >= 0 && term < g.terms && n >= nt * g.BN && n < (nt + 1) * g.BN && k >= g.wk0 &&
                    k + 8 <= g.wk0 + g.K && k % 8 == 0,
                "%s: source term %d n %d k %d", name, term, n, k);
          CHECK(src == ((size_t)term * g.N + n) * g.wstride + k && src % 8 == 0 &&
                    src + 8 <= (size_t)g.terms * g.N * g.wstride,
                "%s: source index %zu", name, src);
          if (src % 8 == 0 && src + 8 <= (size_t)g.terms * g.N * g.wstride) {
            CHECK(!seen_src[src / 8], "%s: source quad %zu twice", name, src / 8);
            seen_src[src / 8] = 1;
          }
          // from the LDS side: where this 16-B unit lands in the K-tile's slot
          const size_t slot = off % wimage_tile_bytes(g);
          const int t_lds = (int)(slot / ((size_t)g.BN * 64));
          const int R = (int)(slot % ((size_t)g.BN * 64) / 64);
          const int p = (int)(slot % 64 / 16);
          const int q = p ^ swz_restated(R);
          CHECK(term == t_lds && n == nt * g.BN + R && k == g.wk0 + wimage_kcol(g, kt) + 8 * q,
                "%s: LDS (term %d row %d quad %d) holds term %d n %d k %d", name, t_lds, R, p, term, n, k);
        }
  size_t n_img = 0, n_src = 0;
  for (unsigned char c : seen_img) n_img += c;
  for (unsigned char c : seen_src) n_src += c;
  CHECK(n_img == bytes / 16, "%s: %zu of %zu image units written", name, n_img, bytes / 16);
  CHECK(n_src == bytes / 16, "%s: %zu source quads read", name, n_src);
  // the MFMA fragment: lane (c16, g) of column block ni reads row 16 ni + c16 at quad g ^ swzB(c16)
  for (int ni = 0; ni < g.BN / 16; ++ni)
    for (int lane = 0; lane < 64; ++lane) {
      const int c16 = lane & 15, gq = lane >> 4;
      const int bfo = c16 * 64 + ((gq ^ wimage_swz(c16)) << 4) + ni * 16 * 64;  // conv_r3_kernel.h bfo
      // the image unit at that slot byte of term 0, K-tile 0, column tile 0
      const int e = bfo / WIMG_PIECE, l = bfo % WIMG_PIECE / 16;
      int term, n, k;
      wimage_source(g, 0, 0, e, l, &term, &n, &k);
      CHECK(term == 0 && n == 16 * ni + c16 && k == g.wk0 + wimage_kcol(g, 0) + 8 * gq,
            "%s: fragment ni %d lane %d reads term %d n %d k %d", name, ni, lane, term, n, k);
    }
  // the waves' pieces: e = wave + NW j
  for (int NW : {4, 8}) {
    std::vector<int> cnt(pieces, 0);
    const int NB = (pieces + NW - 1) / NW, rem = pieces % NW;
    for (int w = 0; w < NW; ++w)
      for (int j = 0; j < NB; ++j)
        if (rem == 0 || j < NB - 1 || w < rem) {
          const int e = w + NW * j;
          CHECK(e < pieces, "%s: wave %d slot %d issues piece %d of %d", name, w, j, e, pieces);
          if (e < pieces) ++cnt[e];
        }
    for (int e = 0; e < pieces; ++e) CHECK(cnt[e] == 1, "%s: NW %d piece %d issued %d times", name, NW, e, cnt[e]);
  }
}

static int dump(char** v) {
  WImageGeom g = {atoi(v[0]), atoi(v[1]), atoi(v[2]), atoi(v[3]), atoi(v[4]), atoi(v[5]), atoi(v[6]), atoi(v[7])};
  if (const char* err = wimage_check(g)) {
    std::printf("refused: %s\n", err);
    return 2;
  }
  std::printf("bytes %zu\n", wimage_bytes(g));
  for (int nt = 0; nt < g.N / g.BN; ++nt)
    for (int kt = 0; kt < wimage_ktiles(g); ++kt)
      for (int e = 0; e < wimage_pieces(g); ++e)
        for (int l = 0; l < 64; ++l) {
          int term, n, k;
          const size_t src = wimage_source(g, nt, kt, e, l, &term, &n, &k);
          std::printf("%zu %d %d %d %zu\n", wimage_offset(g, nt, kt, e, l), term, n, k, src);
        }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 10 && !std::strcmp(argv[1], "dump")) return dump(argv + 2);
  for (int R = 0; R < 1024; ++R) CHECK(wimage_swz(R) == swz_restated(R), "swz(%d)", R);
  // the heads on conv_r3_kernel<256, 320>: chunk-major, levels 2 / 1 / 0 (C = 64 / 128 / 256)
  const WImageGeom heads[3] = {{320, 2304, 2304, 0, 320, 2, 72, 256},
                               {320, 1152, 1152, 0, 320, 2, 36, 128},
                               {320, 576, 576, 0, 320, 2, 18, 64}};
  check_geom(heads[0], "heads L0");
  check_geom(heads[1], "heads L1");
  check_geom(heads[2], "heads L2");
  // conv_r3 128 x 128 body conv: 3x3 (chunk-major) + a fused 1x1 downsample segment (tap-major tail)
  check_geom({128, 9 * 64 + 64, 640, 0, 128, 2, 18, 64}, "layer2 conv + downsample");
  // the same conv tap-major (the strip / conv_h3 families' K order)
  check_geom({128, 9 * 64 + 64, 640, 0, 128, 2, 0, 64}, "tap-major");
  // a K-slice of a wider conv (the commuted FPN W_b half), 64-wide tiles
  check_geom({128, 128, 384, 256, 64, 2, 0, 128}, "FPN slice");
  check_geom({256, 512, 768, 0, 128, 2, 0, 512}, "FPN W_a slice");
  // pieces that do not divide among the waves: BN = 48 -> 6 pieces for 4 or 8 waves
  check_geom({96, 288, 288, 0, 48, 2, 9, 32}, "odd pieces");
  // refused geometries
  CHECK(wimage_check({320, 576, 576, 0, 320, 1, 18, 64}) != nullptr, "one term");
  CHECK(wimage_check({300, 576, 576, 0, 320, 2, 18, 64}) != nullptr, "N % BN");
  CHECK(wimage_check({320, 560, 576, 0, 320, 2, 0, 64}) != nullptr, "K % 32");
  CHECK(wimage_check({320, 576, 576, 4, 320, 2, 0, 64}) != nullptr, "wk0 % 8");
  CHECK(wimage_check({320, 576, 600, 32, 320, 2, 0, 64}) != nullptr, "slice outside the row");
  CHECK(wimage_check({320, 576, 576, 0, 320, 2, 17, 64}) != nullptr, "chunk-major tiles");
  CHECK(wimage_check({320, 576, 576, 0, 320, 2, 18, 48}) != nullptr, "chunk-major C");
  CHECK(wimage_check({64 * 1024, 64 * 1024, 64 * 1024, 0, 64, 2, 0, 64}) != nullptr, "2 GiB");
  // the model's plan: aligned, disjoint, in order
  WImagePlan p;
  CHECK(wimage_plan(heads, 3, &p) == nullptr, "plan");
  size_t end = 0;
  for (int i = 0; i < p.count; ++i) {
    CHECK(p.off[i] % 256 == 0 && p.off[i] >= end && p.bytes[i] == wimage_bytes(heads[i]), "plan region %d", i);
    end = p.off[i] + p.bytes[i];
  }
  CHECK(p.count == 3 && p.total >= end && p.total % 256 == 0, "plan total %zu end %zu", p.total, end);
  CHECK(wimage_plan(heads, WIMG_MAX + 1, &p) != nullptr, "too many images");
  const WImageGeom bad[1] = {{300, 576, 576, 0, 320, 2, 18, 64}};
  CHECK(wimage_plan(bad, 1, &p) != nullptr, "plan of a bad geometry");
  std::printf("wimage_plan_check: %lld checks, %lld bad\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
