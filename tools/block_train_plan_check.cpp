// Host check of csrc/block_train_plan.h, a stand-alone program (its own main) built with -fsanitize=address,undefined
// (tests/test_block_train_host.py): the workspace regions lie apart and inside the size, the split-K chunks and the
// statistics blocks cover every pixel once at caps 0, 3 and 17 with at most kGradBiasMaxBlocks blocks, the forward
// tap source function agrees with a brute-force enumeration (and inverts block_tap_source) for sizes 1 to 41 at both
// strides, and the refusals hold, fewer than 2 values per channel included.
//   g++ -std=c++17 -fsanitize=address,undefined tools/block_train_plan_check.cpp -o block_train_plan_check
#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/block_train_plan.h"
#include "plan_check.h"

using namespace sfa;

static void check_shape(int layer, int block, int B, int h, int w) {
  for (int cap : {0, 3, 17}) {
    BlockTrainForwardPlan f;
    BlockTrainGradPlan g;
    EXPECT(block_train_forward_plan(layer, block, B, h, w, cap, &f), "forward plan L%d.%d %d %d %d", layer, block, B, h, w);
    EXPECT(block_train_grad_plan(layer, block, B, h, w, cap, &g), "grad plan L%d.%d %d %d %d", layer, block, B, h, w);
    const BlockShape& s = f.s;
    const size_t map = (size_t)s.npix_out * s.cout * 4;
    EXPECT(f.nbn == (s.downsample ? 3 : 2) && g.nbn == f.nbn, "BatchNorm count");
    for (const GradBias* st : {&f.st, &g.st}) {
      EXPECT(st->npix == s.npix_out && st->cout == s.cout && st->blocks >= 1 && st->blocks <= kGradBiasMaxBlocks,
             "statistics blocks %d", st->blocks);
      const int least = (s.npix_out + kGradBiasMaxBlocks - 1) / kGradBiasMaxBlocks;
      EXPECT(cap == 0 || st->pixels <= (cap > least ? cap : least) || st->pixels == grad_bias(s.npix_out, s.cout).pixels,
             "cap %d leaves %d pixels", cap, st->pixels);
      check_runs(st->npix, st->pixels, st->blocks, false, "statistics blocks");
    }
    {
      const size_t off[] = {f.off_wk[0], f.off_wk[1], f.off_wk[2], f.off_spart, f.off_coef};
      const size_t len[] = {f.wk_floats[0] * 4, f.wk_floats[1] * 4, f.wk_floats[2] * 4, (size_t)f.st.blocks * s.cout * 16,
                            (size_t)f.nbn * 2 * s.cout * 4};
      EXPECT(f.wk_floats[0] == (size_t)9 * s.cin * s.cout && f.wk_floats[1] == (size_t)9 * s.cout * s.cout &&
                 f.wk_floats[2] == (s.downsample ? (size_t)s.cin * s.cout : 0),
             "weight copies");
      check_regions(off, len, 5, f.total, "forward");
    }
    size_t part = 0;
    for (int i = 0; i < 3; ++i) {
      const BlockWgrad& k = g.wg[i];
      EXPECT(k.Kc >= 1 && (cap == 0 ? k.Kc <= kGradChunkPixels : k.Kc <= cap) && k.npix == s.npix_out, "Kc %d at cap %d", k.Kc, cap);
      EXPECT(k.taps == (i < 2 ? 9 : (s.downsample ? 1 : 0)) && k.rows == s.cout && k.cin == (i == 1 ? s.cout : s.cin), "GEMM %d", i);
      check_runs(k.npix, k.Kc, k.chunks, false, "split-K chunks");
      const size_t bytes = (size_t)k.chunks * k.rows * k.taps * k.cin * 4;
      if (bytes > part) part = bytes;
    }
    {
      const size_t off[] = {g.off_dz2, g.off_dzd, g.off_da, g.off_dz1, g.off_wt[0], g.off_wt[1], g.off_part, g.off_rpart, g.off_sums};
      const size_t len[] = {map, s.downsample ? map : 0, map, map, g.wt_floats[0] * 4, g.wt_floats[1] * 4, part,
                            (size_t)g.st.blocks * s.cout * 16, (size_t)s.cout * 16};
      check_regions(off, len, 9, g.total, "grad");
    }
    ++plans;
  }
}

// one axis of n input cells at stride s
static void check_axis(int n, int s) {
  const int on = (n + s - 1) / s;
  for (int o = 0; o < on; ++o)
    for (int k = 0; k < 3; ++k) {
      int src = -1;
      for (int i = 0; i < n; ++i)
        if (i == o * s - 1 + k) src = i;
      EXPECT(block_train_tap_input(o, k, s, n) == src, "tap input o %d k %d s %d n %d", o, k, s, n);
    }
  // the inverse of the data gradient's source function
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      const int o = block_tap_source(i, k, s, on);
      int brute = -1;
      for (int q = 0; q < on; ++q)
        if (block_train_tap_input(q, k, s, n) == i) brute = q;
      EXPECT(o == brute, "tap source i %d k %d s %d n %d", i, k, s, n);
    }
}

int main() {
  const int shapes[][5] = {{1, 0, 2, 3, 5},  {1, 1, 2, 1, 1},  {1, 1, 1, 2, 70}, {2, 0, 2, 5, 7},     {2, 0, 1, 4, 6},
                           {2, 0, 1, 3, 66}, {2, 0, 2, 2, 2},  {3, 0, 2, 5, 7},  {4, 0, 2, 2, 2},     {4, 1, 2, 3, 5},
                           {3, 1, 1, 2, 70}, {1, 1, 16, 152, 152}, {2, 0, 16, 152, 152}, {4, 1, 16, 19, 19}, {1, 0, 1, 1, 2}};
  for (const auto& s : shapes) check_shape(s[0], s[1], s[2], s[3], s[4]);
  for (int n = 1; n <= 41; ++n)
    for (int s = 1; s <= 2; ++s) check_axis(n, s);
  BlockTrainForwardPlan f;
  BlockTrainGradPlan g;
  // fewer than 2 values per channel: n = B oh ow = 1
  EXPECT(!block_train_forward_plan(1, 0, 1, 1, 1, 0, &f) && !block_train_grad_plan(1, 0, 1, 1, 1, 0, &g), "n = 1 at stride 1");
  EXPECT(!block_train_forward_plan(2, 0, 1, 2, 2, 0, &f) && !block_train_grad_plan(2, 0, 1, 2, 2, 0, &g), "n = 1 at stride 2");
  EXPECT(block_train_forward_plan(2, 0, 2, 2, 2, 0, &f) && block_train_grad_plan(2, 0, 2, 1, 1, 0, &g), "n = 2");
  EXPECT(!block_train_forward_plan(0, 0, 2, 4, 4, 0, &f) && !block_train_forward_plan(5, 0, 2, 4, 4, 0, &f) &&
             !block_train_forward_plan(1, 2, 2, 4, 4, 0, &f) && !block_train_forward_plan(1, -1, 2, 4, 4, 0, &f),
         "layer / block range");
  EXPECT(!block_train_forward_plan(1, 0, 0, 4, 4, 0, &f) && !block_train_forward_plan(1, 0, 2, 0, 4, 0, &f) &&
             !block_train_grad_plan(1, 0, 2, 4, -1, 0, &g),
         "non-positive");
  EXPECT(!block_train_forward_plan(1, 0, 2, 4, 4, -1, &f) && !block_train_grad_plan(1, 0, 2, 4, 4, -1, &g), "negative cap");
  EXPECT(!block_train_forward_plan(1, 0, 1 << 20, 64, 64, 0, &f) && !block_train_grad_plan(4, 1, 1 << 12, 32, 32, 0, &g),
         "a map of 2^31 bytes");
  // a cap below what 256 blocks allow is raised, never the block count
  {
    const GradBias b = block_train_stat_blocks(1000000, 64, 3);
    EXPECT(b.blocks <= kGradBiasMaxBlocks && b.pixels == (1000000 + kGradBiasMaxBlocks - 1) / kGradBiasMaxBlocks, "raised cap");
    const GradBias c = block_train_stat_blocks(70, 64, 3);
    EXPECT(c.pixels == 3 && c.blocks == 24, "cap 3 over 70 pixels");
    const GradBias d = block_train_stat_blocks(70, 64, 0);
    EXPECT(d.pixels == kGradBiasMinPixels && d.blocks == 2, "the plan's own blocks");
  }
  std::printf("%ld plans, %ld bad\n", plans, bad);
  return bad ? 1 : 0;
}
