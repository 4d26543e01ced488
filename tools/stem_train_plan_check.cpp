// Host check of csrc/stem_train_plan.h, a stand-alone program (its own main) built with -fsanitize=address,undefined
// (tests/test_stem_train_host.py): the workspace regions lie apart and inside the size, the split-K chunks and the
// statistics blocks cover every pixel once at caps 0, 3 and 17, conv1's padded K holds whole steps, and the refusals
// hold (n < 2 included).
//   g++ -std=c++17 -fsanitize=address,undefined tools/stem_train_plan_check.cpp -o stem_train_plan_check
#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/stem_train_plan.h"
#include "plan_check.h"

using namespace sfa;

static void check_shape(int B, int H, int W) {
  for (int cap : {0, 3, 17}) {
    StemTrainForwardPlan f;
    StemTrainGradPlan g;
    EXPECT(stem_train_forward_plan(B, H, W, cap, &f) && stem_train_grad_plan(B, H, W, cap, &g), "plans %d %d %d cap %d", B,
           H, W, cap);
    const StemShape& s = g.s;
    EXPECT(s.oh == (H + 6 - 7) / 2 + 1 && s.ow == (W + 6 - 7) / 2 + 1, "conv sizes");
    EXPECT(s.ph == (s.oh + 2 - 3) / 2 + 1 && s.pw == (s.ow + 2 - 3) / 2 + 1, "pool sizes");
    EXPECT(f.s.npix_a == s.npix_a && s.npix_a == B * s.oh * s.ow && s.npix_a >= 2, "pixels");
    EXPECT(g.wg.Kc >= 1 && (cap == 0 ? g.wg.Kc <= kGradChunkPixels : g.wg.Kc <= cap), "Kc %d at cap %d", g.wg.Kc, cap);
    EXPECT(g.wg.npix == s.npix_a && g.wg.rows == kSgC && g.wg.cin == kSgK && g.wg.taps == 1, "dW's GEMM");
    check_runs(g.wg.npix, g.wg.Kc, g.wg.chunks, false, "split-K chunks");
    for (const GradBias* b : {&f.st, &g.st}) {
      EXPECT(b->npix == s.npix_a && b->cout == kSgC && b->blocks >= 1 && b->blocks <= kGradBiasMaxBlocks, "statistics blocks");
      const int own = grad_bias(s.npix_a, kSgC).pixels, least = (s.npix_a + kGradBiasMaxBlocks - 1) / kGradBiasMaxBlocks;
      EXPECT(b->pixels == ((cap > 0 && cap < own) ? (cap > least ? cap : least) : own),
             "a statistics block of %d pixels at cap %d", b->pixels, cap);
      check_runs(b->npix, b->pixels, b->blocks, false, "statistics blocks");
    }
    EXPECT(f.st.pixels == g.st.pixels && f.st.blocks == g.st.blocks, "the forward and the backward share their block order");
    {
      const size_t off[] = {f.off_wk, f.off_spart, f.off_coef};
      const size_t bytes[] = {(size_t)kStKPad * kSgC * 4, (size_t)f.st.blocks * kSgC * 16, (size_t)2 * kSgC * 4};
      check_regions(off, bytes, 3, f.total, "forward");
    }
    {
      const size_t map = (size_t)s.npix_a * kSgC * 4;
      const size_t off[] = {g.off_dy, g.off_dz, g.off_wp, g.off_part, g.off_rpart, g.off_sums};
      const size_t bytes[] = {map, map, (size_t)kSgC * kStWpLd * 4, (size_t)g.wg.chunks * kSgC * kSgK * 4,
                              (size_t)g.st.blocks * kSgC * 16, (size_t)kSgC * 16};
      check_regions(off, bytes, 6, g.total, "grad");
    }
  }
}

int main() {
  const int shapes[][3] = {{1, 3, 3},  {1, 4, 4},   {1, 6, 10},  {2, 12, 20},     {1, 36, 52},    {2, 64, 96},
                           {1, 32, 160}, {3, 7, 9}, {1, 5, 3},   {16, 608, 608},  {1, 40000, 32}, {65535, 3, 3}};
  for (const auto& s : shapes) {
    check_shape(s[0], s[1], s[2]);
    ++plans;
  }
  EXPECT(kStKPad % kGradStep == 0 && kStKPad >= kStK && kStKPad - kStK < kGradStep, "conv1's K in whole steps");
  EXPECT(kStWpLd % 4 == 0 && kStWpLd == 49 * 4, "rows of the data gradient's W copy are float4s");
  StemTrainForwardPlan f;
  StemTrainGradPlan g;
  StemShape s;
  EXPECT(!stem_train_forward_plan(0, 4, 4, 0, &f) && !stem_train_forward_plan(1, 0, 4, 0, &f) &&
             !stem_train_forward_plan(1, 4, -1, 0, &f) && !stem_train_grad_plan(0, 4, 4, 0, &g),
         "non-positive");
  EXPECT(!stem_train_forward_plan(1, 4, 4, -1, &f) && !stem_train_grad_plan(1, 4, 4, -1, &g), "negative cap");
  // n = B oh ow < 2: one conv pixel
  EXPECT(!stem_train_forward_plan(1, 1, 1, 0, &f) && !stem_train_grad_plan(1, 1, 1, 0, &g), "n = 1 at 1 x 1");
  EXPECT(!stem_train_forward_plan(1, 2, 2, 0, &f) && !stem_train_grad_plan(1, 2, 2, 3, &g), "n = 1 at 2 x 2");
  EXPECT(stem_train_forward_plan(2, 1, 1, 0, &f) && stem_train_forward_plan(1, 3, 1, 0, &f), "n = 2");
  // the size limits are the max-pool launch's grid axes, not the fp16x3 convolution's 16-bit packing
  EXPECT(stem_train_shape(1, kSgMaxSide + 1, 4, &s) == 0 && stem_train_shape(1, 4, kSgMaxSide + 1, &s) == 0, "above 32760");
  EXPECT(stem_train_shape(1, kStMaxH, 4, &s) == 0 && s.ph == 65535 && stem_train_shape(1, kStMaxH + 1, 4, &s) == 2, "H limit");
  EXPECT(stem_train_shape(kStMaxBatch, 3, 3, &s) == 0 && stem_train_shape(kStMaxBatch + 1, 3, 3, &s) == 2, "batch limit");
  EXPECT(!stem_train_forward_plan(kStMaxBatch + 1, 3, 3, 0, &f) && !stem_train_grad_plan(1, kStMaxH + 1, 4, 0, &g), "limits refuse");
  // a is the largest map (B oh ow 256 bytes): 2^31 bytes at B oh ow = 2^23
  EXPECT(stem_train_shape(2, 8192, 8192, &s) == 1 && stem_train_shape(32, 1024, 1024, &s) == 1, "2^31-byte map a");
  EXPECT(stem_train_forward_plan(31, 1024, 1024, 0, &f) && stem_train_grad_plan(31, 1024, 1024, 0, &g), "map a below 2^31 bytes");
  EXPECT(stem_train_grad_plan(1, 4096, 4096, 3, &g), "2^30-byte map a at cap 3");
  std::printf("%ld plans, %ld bad\n", plans, bad);
  return bad ? 1 : 0;
}
