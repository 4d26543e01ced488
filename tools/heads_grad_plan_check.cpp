// Host-only check of csrc/heads_grad_plan.h (plain C++: no HIP, no GPU): walks B 1..4, h and w 1..40, the three
// input widths, 1..8 heads and max_chunk_pixels in {0, 1, 7, 64} and checks for every plan that the split-K
// chunks tile every frame's rows exactly once, that no chunk crosses a frame, that K_c is the largest chunk,
// that the column split of the hidden recompute is 128 k + (0 | 64), and that the workspace regions are disjoint, aligned and inside the reported size; then two known answers
// and the refused shapes.  For the same shapes (once per shape, not per chunking) the tiles of heads_dgrad_kernel: every
// pixel of every row and every input channel covered exactly once, the last tile of a row short, never empty; and
// the workspace regions of sfa_model_heads_forward: disjoint, aligned, inside the size.  Built with -fsanitize=address,undefined by tests/test_heads_grad_host.py.
#include <cstdio>
#include <vector>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/heads_grad_plan.h"

using namespace sfa;

static long bad = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      if (bad++ < 20) {              \
        std::printf("BAD: " __VA_ARGS__); \
        std::printf("\n");           \
      }                              \
    }                                \
  } while (0)

static void check_plan(int B, int h, int w, int Cin, int heads, int mcp) {
  HeadsGradPlan p;
  const bool ok = heads_grad_plan(B, h, w, Cin, heads, mcp, &p);
  EXPECT(ok, "refused B %d h %d w %d Cin %d heads %d mcp %d", B, h, w, Cin, heads, mcp);
  if (!ok) return;
  EXPECT(p.M == 64 * heads && p.num_chunks == B * p.chunks_per_frame, "M / chunk count");
  std::vector<int> seen((size_t)B * h, 0);
  int kc = 0;
  for (int c = 0; c < p.num_chunks; ++c) {
    const HeadsGradChunk k = heads_grad_chunk(p, c);
    EXPECT(k.frame >= 0 && k.frame < B && k.rows >= 1 && k.row0 >= 0 && k.row0 + k.rows <= h,
           "chunk %d leaves its frame (frame %d row0 %d rows %d, h %d)", c, k.frame, k.row0, k.rows, h);
    if (k.frame < 0 || k.frame >= B || k.row0 < 0 || k.rows < 0 || k.row0 + k.rows > h) continue;
    for (int r = 0; r < k.rows; ++r) seen[(size_t)k.frame * h + k.row0 + r]++;
    if (k.rows * w > kc) kc = k.rows * w;
    const int cap = mcp > 0 ? mcp : kHgChunkPixels;
    EXPECT(k.rows == 1 || k.rows * w <= cap, "chunk %d of %d pixels above the cap %d", c, k.rows * w, cap);
  }
  for (int v : seen) EXPECT(v == 1, "a row is covered %d times (B %d h %d w %d mcp %d)", v, B, h, w, mcp);
  EXPECT(kc == p.Kc, "K_c %d, largest chunk %d", p.Kc, kc);
  const long long npix = (long long)B * h * w;
  EXPECT((long long)p.dh_blocks * p.dh_pixels >= npix && (long long)(p.dh_blocks - 1) * p.dh_pixels < npix &&
             p.dh_blocks <= kHgDhMaxBlocks + 1 && p.dh_slots == p.M * 5 + heads * 4,
         "dhidden blocks %d x %d pixels for %lld", p.dh_blocks, p.dh_pixels, npix);
  const size_t K = (size_t)9 * Cin;
  const size_t off[7] = {p.off_hidden, p.off_dhidden, p.off_part, p.off_dpart, p.off_terms, p.off_amax, p.total};
  const size_t len[6] = {(size_t)npix * p.M * 4, (size_t)npix * p.M * 4, (size_t)p.num_chunks * p.M * 9 * Cin * 4,
                         (size_t)p.dh_blocks * p.dh_slots * 8, (size_t)2 * p.M * K * 2, (size_t)B * kHgAmaxWords * 4};
  // the column split of the hidden recompute: a multiple of 128, then 0 or 64, together M; both parts inside the
  // hidden and the terms regions
  EXPECT(p.Na % 128 == 0 && (p.Nb == 0 || p.Nb == 64) && p.Na + p.Nb == p.M && p.Na >= 0, "column split %d + %d", p.Na,
         p.Nb);
  EXPECT((size_t)npix * p.Na * 4 + (size_t)npix * p.Nb * 4 == len[0] && 2 * p.Na * K * 2 + 2 * p.Nb * K * 2 == len[4],
         "parts do not fill their regions");
  EXPECT(off[0] == 0, "first region not at 0");
  for (int i = 0; i < 6; ++i) {
    EXPECT(off[i] % kHgAlign == 0, "region %d misaligned", i);
    EXPECT(off[i] + len[i] <= off[i + 1], "region %d overlaps the next / the end", i);
  }
}

static void check_dgrad(int B, int h, int w, int Cin, int heads) {
  HeadsDgradPlan p;
  const bool ok = heads_dgrad_plan(B, h, w, Cin, heads, &p);
  EXPECT(ok, "dgrad refused B %d h %d w %d Cin %d heads %d", B, h, w, Cin, heads);
  if (!ok) return;
  EXPECT(p.tiles_per_row == (w + kHgDgPix - 1) / kHgDgPix && p.chan_tiles * kHgDgCin == Cin &&
             p.blocks == (int64_t)p.tiles_per_row * p.chan_tiles * B * h,
         "dgrad tile counts");
  std::vector<unsigned char> seen((size_t)B * h * w * p.chan_tiles, 0);
  for (int c = 0; c < (int)p.blocks; ++c) {
    const HeadsDgradTile t = heads_dgrad_tile_at(c, w, p.tiles_per_row, p.chan_tiles);
    const bool in = t.row >= 0 && t.row < B * h && t.col0 >= 0 && t.cols >= 1 && t.cols <= kHgDgPix &&
                    t.col0 + t.cols <= w && t.chan0 >= 0 && t.chan0 % kHgDgCin == 0 && t.chan0 + kHgDgCin <= Cin;
    EXPECT(in, "dgrad tile %d leaves the map (row %d col0 %d cols %d chan0 %d; w %d)", c, t.row, t.col0, t.cols, t.chan0, w);
    if (!in) continue;
    EXPECT(t.col0 + t.cols == w || t.cols == kHgDgPix, "dgrad tile %d is short inside a row", c);
    for (int q = 0; q < t.cols; ++q) seen[((size_t)t.row * w + t.col0 + q) * p.chan_tiles + t.chan0 / kHgDgCin]++;
  }
  for (unsigned char v : seen) EXPECT(v == 1, "a dgrad pixel is covered %d times (B %d h %d w %d Cin %d)", (int)v, B, h, w, Cin);
  HeadsForwardPlan f;
  EXPECT(heads_forward_plan(B, h, w, Cin, heads, &f), "forward plan refused");
  const size_t npix = (size_t)B * h * w;
  const size_t off[4] = {f.off_hidden, f.off_terms, f.off_amax, f.total};
  const size_t len[3] = {npix * f.M * 4, (size_t)2 * f.M * 9 * Cin * 2, (size_t)B * kHgAmaxWords * 4};
  EXPECT(f.M == 64 * heads && f.Na + f.Nb == f.M && f.Na % 128 == 0 && off[0] == 0, "forward plan columns");
  for (int i = 0; i < 3; ++i) {
    EXPECT(off[i] % kHgAlign == 0, "forward region %d misaligned", i);
    EXPECT(off[i] + len[i] <= off[i + 1], "forward region %d overlaps the next / the end", i);
  }
}

int main() {
  long plans = 0;
  const int cins[3] = {256, 128, 64}, mcps[4] = {0, 1, 7, 64};
  for (int B = 1; B <= 4; ++B)
    for (int h = 1; h <= 40; ++h)
      for (int w = 1; w <= 40; ++w)
        for (int Cin : cins)
          for (int heads = 1; heads <= 8; ++heads)
          {
            for (int mcp : mcps) {
              check_plan(B, h, w, Cin, heads, mcp);
              ++plans;
            }
            check_dgrad(B, h, w, Cin, heads);
          }
  // widths around the dgrad pixel tile: one short, exact, one over, two tiles + 5
  for (int w : {kHgDgPix - 1, kHgDgPix, kHgDgPix + 1, 2 * kHgDgPix + 5, 152})
    for (int Cin : cins) check_dgrad(2, 3, w, Cin, 5);
  // known answers, by hand.  B 2, 6 x 8, Cin 128, 5 heads, cap 7: one row per chunk, 6 chunks per frame, K_c 8;
  // 96 pixels in 3 blocks of 32; regions 96 * 320 * 4 = 122880 (= 480 * 256) twice, 12 * 320 * 9 * 128 * 4 =
  // 17694720 (= 69120 * 256), 3 * 1620 * 8 = 38880 -> 38912, the fp16 terms 2 * 320 * 1152 * 2 = 1474560 (= 5760 * 256),
  // the two frames' max records 2 * 256 * 4 = 2048; columns 256 + 64.
  HeadsGradPlan p;
  EXPECT(heads_grad_plan(2, 6, 8, 128, 5, 7, &p), "known answer 1 refused");
  EXPECT(p.rows_per_chunk == 1 && p.chunks_per_frame == 6 && p.num_chunks == 12 && p.Kc == 8, "known answer 1 chunks");
  EXPECT(p.dh_pixels == 32 && p.dh_blocks == 3 && p.dh_slots == 1620, "known answer 1 dhidden");
  EXPECT(p.off_hidden == 0 && p.off_dhidden == 122880 && p.off_part == 245760 && p.off_dpart == 17940480 &&
             p.off_terms == 17979392 && p.off_amax == 19453952 && p.total == 19456000 && p.Na == 256 && p.Nb == 64,
         "known answer 1 regions (%zu %zu %zu %zu %zu %zu)", p.off_dhidden, p.off_part, p.off_dpart, p.off_terms,
         p.off_amax, p.total);
  const HeadsGradChunk k7 = heads_grad_chunk(p, 7);
  EXPECT(k7.frame == 1 && k7.row0 == 1 && k7.rows == 1, "known answer 1 chunk 7");
  // B 16, 152 x 152, Cin 64, 5 heads, own choice: 4096 / 152 = 26 rows, 6 chunks per frame (the last of 22 rows),
  // K_c 3952; 369664 pixels -> 361 per block (ceil(369664 / 1024)), 1024 blocks.
  EXPECT(heads_grad_plan(16, 152, 152, 64, 5, 0, &p), "known answer 2 refused");
  EXPECT(p.rows_per_chunk == 26 && p.chunks_per_frame == 6 && p.num_chunks == 96 && p.Kc == 3952, "known answer 2 chunks");
  EXPECT(p.dh_pixels == 361 && p.dh_blocks == 1024, "known answer 2 dhidden (%d, %d)", p.dh_pixels, p.dh_blocks);
  const HeadsGradChunk k5 = heads_grad_chunk(p, 5), k6 = heads_grad_chunk(p, 6);
  EXPECT(k5.frame == 0 && k5.row0 == 130 && k5.rows == 22 && k6.frame == 1 && k6.row0 == 0 && k6.rows == 26,
         "known answer 2 chunks 5, 6");
  // dgrad known answer, by hand: 16 frames of 152 x 152 at Cin 128: 3 tiles per row (64, 64, 24), 2 channel tiles,
  // 16 * 152 * 6 = 14592 blocks; block 11 = channel tile 1 of pixel tile 2 of row 1
  HeadsDgradPlan dp;
  EXPECT(heads_dgrad_plan(16, 152, 152, 128, 5, &dp) && dp.tiles_per_row == 3 && dp.chan_tiles == 2 && dp.blocks == 14592,
         "dgrad known answer counts");
  const HeadsDgradTile t11 = heads_dgrad_tile_at(11, 152, 3, 2);
  EXPECT(t11.row == 1 && t11.col0 == 128 && t11.cols == 24 && t11.chan0 == 64, "dgrad known answer tile 11");
  HeadsForwardPlan fp;
  EXPECT(heads_forward_plan(2, 6, 8, 128, 5, &fp) && fp.off_terms == 122880 && fp.off_amax == 122880 + 1474560 &&
             fp.total == 122880 + 1474560 + 2048 && fp.Na == 256 && fp.Nb == 64,
         "forward plan known answer");
  EXPECT(!heads_dgrad_plan(0, 4, 4, 64, 5, &dp) && !heads_dgrad_plan(1, 4, 4, 48, 5, &dp) &&
             !heads_dgrad_plan(64, 512, 512, 64, 5, &dp) && !heads_forward_plan(1, 4, 0, 64, 5, &fp),
         "dgrad / forward refusals");
  // refused
  EXPECT(!heads_grad_plan(0, 4, 4, 64, 5, 0, &p) && !heads_grad_plan(1, 0, 4, 64, 5, 0, &p) &&
             !heads_grad_plan(1, 4, -1, 64, 5, 0, &p) && !heads_grad_plan(1, 4, 4, 48, 5, 0, &p) &&
             !heads_grad_plan(1, 4, 4, 64, 0, 0, &p) && !heads_grad_plan(1, 4, 4, 64, 9, 0, &p) &&
             !heads_grad_plan(1, 4, 4, 64, 5, -1, &p) && !heads_grad_plan(64, 512, 512, 64, 5, 0, &p) &&
             heads_grad_plan(16, 152, 152, 256, 8, 0, &p),
         "refusals");
  std::printf("%ld plans, %ld bad\n", plans, bad);
  return bad ? 1 : 0;
}
