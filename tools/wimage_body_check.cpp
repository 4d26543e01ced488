// Stand-alone host check of the body convs' pre-tiled weight images (csrc/conv_wimage.h: the strip K order,
// split-K slices, the body plan; csrc/conv_plan.h: strip_tile_bn, conv_h3s_image_check):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/wimage_body_check.cpp -o /tmp/wimage_body_check
//   /tmp/wimage_body_check                 # the self-check: "wimage_body_check: N checks, 0 bad"
//   /tmp/wimage_body_check dump N K wstride wk0 BN terms cmaj_tiles C strip
//                                          # one line "offset term n k src" per (nt, kt, e, lane), in image order
// Walked from the LDS side (per term, rows of 64 B, source quad q of row R at quad q ^ swzB(R)), for layer1
// (C = 64, BN = 64), a 128 x 128 strip conv, the 64 x 128 layer3 instance, a split-K 2 strip conv (both
// slices), the two-segment layer2.0 conv (chunk-major + a 1x1 tail), a stride-2 conv_h3 conv with slices
// (tap-major) and a tile whose pieces do not divide among the waves:
//  * the image is dense, every source quad is read exactly once and lies inside the terms;
//  * the fragment formula holds (the lane of a column block reads k = 8 g .. 8 g + 7 of its row);
//  * strip convs: the offset conv_h3s_kernel<.., h3sopt::W_IMAGE> computes for (slice, super-step, kw, wave,
//    slot, lane) is wimage_offset of that K-tile and piece, inside the image, and holds the 16 bytes the
//    row-major path's offset (boff + 2 wk0) reads for the same LDS bytes; a slice's K-tiles are contiguous
//    and the slices partition the conv's;
//  * the body plan's regions are 256-B aligned and disjoint, its cap is its own, the heads' cap is unchanged;
//  * wrong geometries and images of another size or tile width are refused.
// Only the strip family's kernels read an image today; the other two geometries are walked for the plan.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/conv_plan.h"

namespace sfa {
static char g_err[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
}  // namespace sfa
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

// the kernels' swizzle, from the comment's words: bits 2..3 of the row, xor'ed with whether (row % 16) + 4
// has bit 3 set
static int swz_restated(int R) { return ((R / 4) % 4) ^ (((R % 16) + 4) / 8 % 2); }

// the K order restated per family: first weight column of K-tile kt
static int kcol_restated(const WImageGeom& g, int kt) {
  if (g.strip) {  // (kh, chunk, kw): kw fastest, then the 32-channel chunk, then kh
    const int nchunk = g.C / 32;
    const int kw = kt % 3, chunk = (kt / 3) % nchunk, kh = kt / 3 / nchunk;
    return (kh * 3 + kw) * g.C + chunk * 32;
  }
  if (kt < g.cmaj_tiles) return (kt % 9) * g.C + (kt / 9) * 32;
  return kt * 32;
}

static void check_geom(const WImageGeom& g, const char* name) {
  CHECK(wimage_check(g) == nullptr, "%s: %s", name, wimage_check(g));
  if (wimage_check(g)) return;
  const int ntile = g.N / g.BN, kt_n = wimage_ktiles(g), pieces = wimage_pieces(g);
  const size_t bytes = wimage_bytes(g);
  CHECK(bytes == (size_t)g.terms * g.N * g.K * 2, "%s: image %zu bytes", name, bytes);
  std::vector<unsigned char> seen_img(bytes / 16, 0);
  std::vector<unsigned char> seen_src((size_t)g.terms * g.N * (g.wstride / 8), 0);
  std::vector<int> kcols(kt_n, 0);
  for (int kt = 0; kt < kt_n; ++kt) {
    const int kc = wimage_kcol(g, kt);
    CHECK(kc == kcol_restated(g, kt), "%s: kcol(%d) = %d", name, kt, kc);
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
          const bool in_terms = src % 8 == 0 && src + 8 <= (size_t)g.terms * g.N * g.wstride;
          CHECK(src == ((size_t)term * g.N + n) * g.wstride + k && in_terms, "%s: source index %zu", name, src);
          if (in_terms) {
            CHECK(!seen_src[src / 8], "%s: source quad %zu twice", name, src / 8);
            seen_src[src / 8] = 1;
          }
          // from the LDS side: where this 16-B unit lands in the K-tile's slot
          const size_t slot = off % wimage_tile_bytes(g);
          const int t_lds = (int)(slot / ((size_t)g.BN * 64));
          const int R = (int)(slot % ((size_t)g.BN * 64) / 64);
          const int p = (int)(slot % 64 / 16);
          const int q = p ^ swz_restated(R);
          CHECK(term == t_lds && n == nt * g.BN + R && k == g.wk0 + kcol_restated(g, kt) + 8 * q,
                "%s: LDS (term %d row %d quad %d) holds term %d n %d k %d", name, t_lds, R, p, term, n, k);
        }
  size_t n_img = 0, n_src = 0;
  for (unsigned char c : seen_img) n_img += c;
  for (unsigned char c : seen_src) n_src += c;
  CHECK(n_img == bytes / 16, "%s: %zu of %zu image units written", name, n_img, bytes / 16);
  CHECK(n_src == bytes / 16, "%s: %zu source quads read", name, n_src);
  // the MFMA fragment (conv_h3s_kernel.h compute: SB + ni * 16 * BROW): lane (c16, g) of column block ni
  // reads row 16 ni + c16 at quad g ^ swzB(c16), of every K-tile
  for (int kt = 0; kt < kt_n; ++kt)
    for (int ni = 0; ni < g.BN / 16; ++ni)
      for (int lane = 0; lane < 64; ++lane) {
        const int c16 = lane & 15, gq = lane >> 4;
        const int bfo = c16 * 64 + ((gq ^ swz_restated(c16)) << 4) + ni * 16 * 64;
        for (int t = 0; t < g.terms; ++t) {
          const int byte = t * g.BN * 64 + bfo;
          int term, n, k;
          wimage_source(g, 0, kt, byte / WIMG_PIECE, byte % WIMG_PIECE / 16, &term, &n, &k);
          CHECK(term == t && n == 16 * ni + c16 && k == g.wk0 + kcol_restated(g, kt) + 8 * gq,
                "%s: fragment kt %d ni %d lane %d term %d reads term %d n %d k %d", name, kt, ni, lane, t, term, n, k);
        }
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

// conv_h3s_kernel<BM, BN, WM, .., h3sopt::W_IMAGE> of a conv of N x 9 C at `nsplit` slices, restated: what
// each (block column nt, slice kz, super-step, kw, wave, slot jj, lane) reads, against the image's index
// function and against the row-major path's source for the same LDS bytes (piece e at e * 1024 + 16 lane).
static void check_strip_kernel(int N, int C, int BN, int NW, int nsplit, const char* name) {
  const int Kpad = 9 * C;
  const WImageGeom g = {N, Kpad, Kpad, 0, BN, 2, 0, C, 1};
  check_geom(g, name);
  if (wimage_check(g)) return;
  const int ND_B = 2 * BN * 64 / 1024, W_BYTES = ND_B * 1024;
  const int NB = (ND_B + NW - 1) / NW, NB_REM = ND_B % NW;
  const int nchunk = C / 32, nsl = 3 * nchunk / nsplit;
  CHECK(3 * nchunk % nsplit == 0, "%s: slices", name);
  const size_t bytes = wimage_bytes(g);
  const unsigned term_bytes = (unsigned)N * Kpad * 2u;
  std::vector<int> tile_seen(Kpad / 32, 0);
  for (int nt = 0; nt < N / BN; ++nt)
    for (int kz = 0; kz < nsplit; ++kz) {
      const int s0 = kz * nsl;
      int prev_kt = -1;
      for (int sl = 0; sl < nsl; ++sl)
        for (int kw = 0; kw < 3; ++kw) {
          const int s = s0 + sl;
          const int kt = 3 * s + kw;                                  // the kernel's wk0 with the image
          const int kh = s / nchunk, c0 = (s % nchunk) * 32;
          const int k0 = (kh * 3 + kw) * C + c0;                      // ... and without
          CHECK(prev_kt < 0 || kt == prev_kt + 1, "%s: slice %d K-tiles not contiguous at %d", name, kz, kt);
          CHECK(kt >= 3 * s0 && kt < 3 * (s0 + nsl), "%s: slice %d K-tile %d", name, kz, kt);
          prev_kt = kt;
          if (nt == 0) ++tile_seen[kt];
          for (int wave = 0; wave < NW; ++wave)
            for (int jj = 0; jj < NB; ++jj) {
              if (!(NB_REM == 0 || jj < NB - 1 || wave < NB_REM)) continue;
              const int e = wave + NW * jj;
              for (int lane = 0; lane < 64; ++lane) {
                const long long wlane = 16 * lane + ((long long)nt * (Kpad >> 5) * ND_B + wave) * 1024;
                const long long off = wlane + (long long)kt * W_BYTES + (long long)NW * jj * 1024;
                CHECK(off >= 0 && off + 16 <= (long long)bytes && off < (1ll << 31), "%s: offset %lld", name, off);
                CHECK((size_t)off == wimage_offset(g, nt, kt, e, lane), "%s: kernel offset %lld != image %zu", name, off,
                      wimage_offset(g, nt, kt, e, lane));
                // the row-major path (boff[jj] + 2 k0), in bytes of the terms
                const int term = e / (ND_B / 2);
                const int R = (e - term * (ND_B / 2)) * 16 + (lane >> 2);
                const int lc = (lane & 3) ^ swz_restated(R);
                const long long row_major =
                    (long long)term * term_bytes + (((long long)(nt * BN + R) * Kpad + 8 * lc) << 1) + 2 * k0;
                CHECK(row_major == 2 * (long long)wimage_source(g, nt, kt, e, lane, nullptr, nullptr, nullptr),
                      "%s: nt %d kt %d piece %d lane %d: image holds another quad than the row-major read", name, nt,
                      kt, e, lane);
              }
            }
        }
    }
  for (int kt = 0; kt < Kpad / 32; ++kt) CHECK(tile_seen[kt] == 1, "%s: K-tile %d swept %d times", name, kt, tile_seen[kt]);
}

static float g_mem[4];

// a strip conv's launch arguments (what the checks read)
static ConvArgs strip_args(int N, int C, int H, int W) {
  ConvArgs a;
  std::memset(&a, 0, sizeof a);
  a.nseg = 1;
  a.seg[0].x = g_mem;
  a.seg[0].H = H;
  a.seg[0].W = W;
  a.seg[0].C = C;
  a.seg[0].KH = a.seg[0].KW = 3;
  a.seg[0].stride = 1;
  a.seg[0].pad = 1;
  a.Kpad = 9 * C;
  a.N = N;
  a.OH = H;
  a.OW = W;
  a.M = H * W;
  a.wh = reinterpret_cast<const uint16_t*>(g_mem);
  a.winv = g_mem;
  a.bias = g_mem;
  a.part = g_mem;
  return a;
}

static int dump(char** v) {
  WImageGeom g = {atoi(v[0]), atoi(v[1]), atoi(v[2]), atoi(v[3]), atoi(v[4]),
                  atoi(v[5]), atoi(v[6]), atoi(v[7]), atoi(v[8])};
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
  if (argc == 11 && !std::strcmp(argv[1], "dump")) return dump(argv + 2);
  for (int R = 0; R < 1024; ++R) CHECK(wimage_swz(R) == swz_restated(R), "swz(%d)", R);
  // the strip family: <128, 64, 32> (4 waves), <128, 128, 32> (4 waves), <64, 128, 16> (4 waves)
  check_strip_kernel(64, 64, 64, 4, 1, "layer1 128x64");
  check_strip_kernel(128, 128, 128, 4, 1, "layer2 128x128");
  check_strip_kernel(256, 256, 128, 4, 1, "layer3 64x128");
  check_strip_kernel(512, 512, 64, 4, 2, "layer4 128x64 split-K 2");
  check_strip_kernel(128, 64, 128, 4, 3, "split-K 3 of 6 super-steps");
  // pieces that do not divide among the waves: BN = 48 -> 6 pieces for 4 (and 8) waves
  check_strip_kernel(96, 32, 48, 4, 1, "odd pieces 4 waves");
  check_strip_kernel(96, 32, 48, 8, 1, "odd pieces 8 waves");
  // the other two body families' geometries (no kernel of theirs reads an image yet): layer2.0 conv2 + the 1x1
  // downsample (chunk-major 3x3 of 128 channels, then the tap-major tail of 64), and a stride-2 conv_h3 conv
  // (tap-major), whose split-K slice z of 2 sweeps K-tiles [z ktiles / 2, (z + 1) ktiles / 2)
  check_geom({128, 9 * 128 + 64, 9 * 128 + 64, 0, 128, 2, 36, 128, 0}, "layer2.0 conv2 + downsample");
  {
    const WImageGeom g = {256, 9 * 128, 9 * 128, 0, 128, 2, 0, 128, 0};
    check_geom(g, "layer3.0 conv1 stride 2");
    const int kt_n = wimage_ktiles(g);
    for (int z = 0; z < 2; ++z)
      for (int kt = z * kt_n / 2; kt < (z + 1) * kt_n / 2; ++kt)
        CHECK(wimage_offset(g, 0, kt, 0, 0) == (size_t)kt * wimage_tile_bytes(g) && wimage_kcol(g, kt) == 32 * kt,
              "conv_h3 slice %d K-tile %d", z, kt);
  }
  // refused geometries of the strip order
  CHECK(wimage_check({64, 576, 576, 0, 64, 2, 0, 64, 1}) == nullptr, "strip geometry");
  CHECK(wimage_check({64, 576 + 64, 640, 0, 64, 2, 0, 64, 1}) != nullptr, "strip with a tail segment");
  CHECK(wimage_check({64, 576, 576, 0, 64, 2, 18, 64, 1}) != nullptr, "strip and chunk-major");
  CHECK(wimage_check({64, 432, 432, 0, 64, 2, 0, 48, 1}) != nullptr, "strip C %% 32");
  CHECK(wimage_check({64, 576, 576, 0, 64, 1, 0, 64, 1}) != nullptr, "strip one term");
  CHECK(wimage_check({64, 576, 576, 0, 48, 2, 0, 64, 1}) != nullptr, "strip N %% BN");
  // zero-initialised trailing field: the orders of before
  {
    const WImageGeom old8 = {128, 640, 640, 0, 128, 2, 18, 64};
    CHECK(old8.strip == 0 && wimage_kcol(old8, 1) == 64 && wimage_kcol(old8, 19) == 19 * 32, "eight-value initialiser");
  }
  // the launch check: the image must be the instance's
  {
    ConvArgs a = strip_args(64, 64, 152, 152);
    const WImageGeom g = conv_h3s_image_geom(a, 64);
    CHECK(g.strip == 1 && g.BN == 64 && g.K == 576 && g.C == 64, "instance geometry");
    a.wimg = reinterpret_cast<const unsigned char*>(g_mem);
    a.wimg_bytes = (unsigned)wimage_bytes(g);
    a.wimg_bn = 64;
    CHECK(conv_h3s_image_check(a, 64) == SFA_OK, "fitting image: %s", g_err);
    a.wimg_bn = 128;
    CHECK(conv_h3s_image_check(a, 64) == SFA_E_INVALID, "another tile width");
    a.wimg_bn = 64;
    a.wimg_bytes -= 1024;
    CHECK(conv_h3s_image_check(a, 64) == SFA_E_INVALID, "another size");
    a.wimg_bytes += 1024;
    a.wimg = nullptr;
    CHECK(conv_h3s_image_check(a, 64) == SFA_E_INVALID, "no image");
    a.wimg = reinterpret_cast<const unsigned char*>(g_mem);
    CHECK(conv_h3s_image_check(a, 48) == SFA_E_INVALID, "N %% BN");
  }
  // strip_tile_bn: the tile width conv.hip's rules give the model's strip convs at 608 x 608 (maps of 152,
  // 76, 38, 19), none for maps of under 128 rows, stride 2 or K-slices; 128-wide layer4 tiles on large maps
  CHECK(strip_tile_bn(strip_args(64, 64, 152, 152)) == 64, "layer1");
  CHECK(strip_tile_bn(strip_args(128, 128, 76, 76)) == 128, "layer2");
  CHECK(strip_tile_bn(strip_args(256, 256, 38, 38)) == 128, "layer3");
  CHECK(strip_tile_bn(strip_args(512, 512, 19, 19)) == 64, "layer4");
  CHECK(strip_tile_bn(strip_args(512, 512, 64, 64)) == 128, "layer4 on a large map");
  CHECK(strip_tile_bn(strip_args(256, 256, 10, 10)) == 0, "frames under 128 rows");
  {
    ConvArgs a = strip_args(128, 128, 76, 76);
    a.seg[0].stride = 2;
    CHECK(strip_tile_bn(a) == 0, "stride 2");
    a = strip_args(128, 128, 76, 76);
    a.wstride = 2 * a.Kpad;
    CHECK(strip_tile_bn(a) == 0, "K-slice");
    a = strip_args(512, 512, 19, 19);
    a.part = nullptr;  // no split-K workspace: one slice, 128-wide tiles
    CHECK(strip_tile_bn(a) == 128, "layer4 without split-K");
  }
  // the body plan: the model's ten strip convs; aligned, disjoint, in order; a cap of its own
  {
    std::vector<WImageGeom> body;
    for (int li = 0; li < 4; ++li)
      for (int k = 0; k < 4; ++k) {
        if (li > 0 && k < 2) continue;
        const int C = 64 << li, BN = (C == 64 || C == 512) ? 64 : 128;
        body.push_back({C, 9 * C, 9 * C, 0, BN, 2, 0, C, 1});
      }
    CHECK(body.size() == 10, "ten strip convs");
    WBodyImagePlan p;
    CHECK(wimage_plan(body.data(), (int)body.size(), &p) == nullptr, "body plan");
    size_t end = 0;
    for (int i = 0; i < p.count; ++i) {
      CHECK(p.off[i] % 256 == 0 && p.off[i] >= end && p.bytes[i] == wimage_bytes(body[i]), "body plan region %d", i);
      end = p.off[i] + p.bytes[i];
    }
    CHECK(p.count == 10 && p.total >= end && p.total % 256 == 0, "body plan total %zu end %zu", p.total, end);
    WImagePlan heads_plan;
    CHECK(wimage_plan(body.data(), (int)body.size(), &heads_plan) != nullptr && WIMG_MAX == 8, "the heads' cap stays 8");
    std::vector<WImageGeom> many(WIMG_BODY_MAX + 1, body[0]);
    CHECK(wimage_plan(many.data(), WIMG_BODY_MAX + 1, &p) != nullptr, "too many body images");
    CHECK(wimage_plan(many.data(), WIMG_BODY_MAX, &p) == nullptr, "the body cap");
    many[3].K = 560;
    CHECK(wimage_plan(many.data(), 4, &p) != nullptr, "body plan of a bad geometry");
  }
  std::printf("wimage_body_check: %lld checks, %lld bad\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
