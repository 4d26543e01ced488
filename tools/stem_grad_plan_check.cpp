// Host check of csrc/stem_grad_plan.h, a stand-alone program (its own main) built with -fsanitize=address,undefined
// (tests/test_stem_host.py): the workspace regions lie apart and inside the size, the split-K chunks and the bias blocks
// cover every pixel once at caps 0, 3 and 17, the window / tap source functions agree with a brute-force enumeration at
// odd and even sizes, and the refusals hold.
//   g++ -std=c++17 -fsanitize=address,undefined tools/stem_grad_plan_check.cpp -o stem_grad_plan_check
#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/stem_grad_plan.h"
#include "plan_check.h"

using namespace sfa;

static void check_shape(int B, int H, int W) {
  StemForwardPlan f;
  EXPECT(stem_forward_plan(B, H, W, &f), "forward plan %d %d %d", B, H, W);
  const StemShape& s = f.s;
  EXPECT(s.oh == (H + 6 - 7) / 2 + 1 && s.ow == (W + 6 - 7) / 2 + 1, "conv sizes");
  EXPECT(s.ph == (s.oh + 2 - 3) / 2 + 1 && s.pw == (s.ow + 2 - 3) / 2 + 1, "pool sizes");
  {
    const size_t off[] = {f.off_xin, f.off_amax}, bytes[] = {(size_t)s.npix_x * 16, f.amax_bytes};
    check_regions(off, bytes, 2, f.total, "forward");
  }
  for (int cap : {0, 3, 17}) {
    StemGradPlan g;
    EXPECT(stem_grad_plan(B, H, W, cap, &g), "grad plan");
    EXPECT(g.wg.Kc >= 1 && (cap == 0 ? g.wg.Kc <= kGradChunkPixels : g.wg.Kc <= cap), "Kc %d at cap %d", g.wg.Kc, cap);
    EXPECT(g.wg.npix == s.npix_a && g.bs.npix == s.npix_a && g.bs.blocks <= kGradBiasMaxBlocks, "pixels of the runs");
    check_runs(g.wg.npix, g.wg.Kc, g.wg.chunks, false, "split-K chunks");
    check_runs(g.bs.npix, g.bs.pixels, g.bs.blocks, false, "bias blocks");
    const size_t off[] = {g.off_da, g.off_part, g.off_bpart};
    const size_t bytes[] = {(size_t)s.npix_a * kSgC * 4, (size_t)g.wg.chunks * kSgC * kSgK * 4, (size_t)g.bs.blocks * kSgC * 8};
    check_regions(off, bytes, 3, g.total, "grad");
  }
}

// one axis of n image cells: on conv outputs, pn pool windows
static void check_axis(int n) {
  const int on = (n + 1) / 2, pn = (on + 1) / 2;
  // pool: brute force which windows hold conv index i
  for (int i = 0; i < on; ++i) {
    std::vector<int> holds;
    for (int v = 0; v < pn; ++v)
      if (i >= 2 * v - 1 && i <= 2 * v + 1) holds.push_back(v);
    const int first = stem_pool_first_window(i), cnt = stem_pool_windows(i, pn);
    EXPECT((int)holds.size() == cnt && holds[0] == first && holds.back() == first + cnt - 1, "windows of %d in %d", i, on);
  }
  // conv: brute force which (tap, output) pairs reach image index i
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 7; ++k) {
      int src = -1;
      for (int o = 0; o < on; ++o)
        if (2 * o - 3 + k == i) src = o;
      EXPECT(stem_tap_source(i, k, on) == src, "tap source i %d k %d", i, k);
      if (src >= 0) EXPECT((k - stem_first_tap(i)) % 2 == 0 && k >= stem_first_tap(i), "parity i %d k %d", i, k);
    }
  }
  for (int j = 0; j < kSgK; ++j) {
    int c, ky, kx;
    stem_column(j, &c, &ky, &kx);
    EXPECT(c >= 0 && c < 3 && ky >= 0 && ky < 7 && kx >= 0 && kx < 7 && (c * 7 + ky) * 7 + kx == j, "column %d", j);
  }
}

int main() {
  const int shapes[][3] = {{1, 1, 1}, {1, 4, 4}, {1, 6, 10}, {2, 12, 20}, {1, 36, 52}, {2, 64, 96}, {1, 32, 160},
                           {3, 7, 9},  {1, 5, 3}, {16, 608, 608}, {1, 32760, 32}, {65535, 2, 2}};
  for (const auto& s : shapes) {
    check_shape(s[0], s[1], s[2]);
    ++plans;
  }
  for (int n = 1; n <= 41; ++n) check_axis(n);
  StemForwardPlan f;
  StemGradPlan g;
  EXPECT(!stem_forward_plan(0, 4, 4, &f) && !stem_forward_plan(1, 0, 4, &f) && !stem_forward_plan(1, 4, -1, &f), "non-positive");
  EXPECT(!stem_forward_plan(1, kSgMaxSide + 1, 4, &f) && !stem_forward_plan(1, 4, kSgMaxSide + 1, &f), "side limit");
  EXPECT(stem_forward_plan(1, kSgMaxSide, 4, &f), "largest side");
  EXPECT(!stem_forward_plan(kSgMaxBatch + 1, 4, 4, &f), "batch limit");
  EXPECT(!stem_grad_plan(1, 4, 4, -1, &g), "negative cap");
  // a is the largest map (B oh ow 256 bytes against the image's B H W 16 as NHWC4): 2^31 bytes at B oh ow = 2^23
  EXPECT(!stem_forward_plan(2, 8192, 8192, &f) && !stem_grad_plan(2, 8192, 8192, 0, &g), "2^33-byte map a");
  EXPECT(!stem_forward_plan(32, 1024, 1024, &f) && !stem_grad_plan(32, 1024, 1024, 0, &g), "2^31-byte map a");
  EXPECT(stem_forward_plan(31, 1024, 1024, &f) && stem_grad_plan(31, 1024, 1024, 0, &g), "map a below 2^31 bytes");
  EXPECT(stem_forward_plan(1, 4096, 4096, &f) && stem_grad_plan(1, 4096, 4096, 3, &g), "2^30-byte map a");
  std::printf("%ld plans, %ld bad\n", plans, bad);
  return bad ? 1 : 0;
}
