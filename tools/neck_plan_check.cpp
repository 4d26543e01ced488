// Host-only check of csrc/neck_plan.h (plain C++: no HIP, no GPU): walks B 1..3, h4 and w4 1..9 and max_chunk_pixels
// in {0, 1, 7, 64, 5000} and checks for every plan that the pixel tiles of the four resolutions and the channel
// tiles of every GEMM cover every pixel and channel exactly once (the last tile short, never empty), that the split-K
// chunks of the four weight gradients and the blocks of the three bias gradients partition their pixels, that K_c
// is the largest chunk and within the cap, and that the workspace regions of both entries are disjoint, aligned and
// inside the reported size; then two known answers computed by hand and the refused shapes.  Built with
// -fsanitize=address,undefined by tests/test_neck_host.py.
#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/neck_plan.h"
#include "plan_check.h"

using namespace sfa;

static void check_plan(int B, int h4, int w4, int mcp) {
  NeckGradPlan p;
  NeckForwardPlan f;
  const bool ok = neck_grad_plan(B, h4, w4, mcp, &p) && neck_forward_plan(B, h4, w4, &f);
  EXPECT(ok, "refused B %d h4 %d w4 %d mcp %d", B, h4, w4, mcp);
  if (!ok) return;
  ++plans;
  for (int r = 0; r < 4; ++r) {
    EXPECT(p.npix[r] == (B * h4 * w4) << (2 * r) && f.npix[r] == p.npix[r], "npix[%d] %d", r, p.npix[r]);
    check_runs(p.npix[r], kGradTile, grad_tiles(p.npix[r]), true, "pixel tiles");
  }
  const int cap = mcp > 0 ? mcp : kGradChunkPixels;
  const int rows[4] = {256, 256, 128, 64}, cols[4] = {512, 256, 384, 192};
  size_t part = 0, bpart = 0;
  for (int i = 0; i < 4; ++i) {
    const NeckWgrad& g = p.wg[i];
    EXPECT(g.rows == rows[i] && g.cols == cols[i] && g.npix == p.npix[i] && g.rows % kGradTile == 0 && g.cols % kGradTile == 0,
           "wgrad %d: %d x %d over %d", i, g.rows, g.cols, g.npix);
    EXPECT(g.Kc >= 1 && g.Kc <= cap && g.Kc <= g.npix && (g.Kc == cap || g.Kc == g.npix), "wgrad %d: K_c %d, cap %d", i, g.Kc,
           cap);
    check_runs(g.npix, g.Kc, g.chunks, false, "split-K chunks");
    check_runs(g.rows, kGradTile, grad_tiles(g.rows), true, "row tiles");
    check_runs(g.cols, kGradTile, grad_tiles(g.cols), true, "column tiles");
    const size_t bytes = (size_t)g.chunks * g.rows * g.cols * 4;
    if (bytes > part) part = bytes;
  }
  for (int s = 0; s < 3; ++s) {
    const GradBias& b = p.bs[s];
    EXPECT(b.npix == p.npix[s + 1] && b.cout == kNkCout[s] && b.cout <= 256 && b.pixels >= kGradBiasMinPixels &&
               b.blocks >= 1 && b.blocks <= kGradBiasMaxBlocks,
           "bias %d: %d blocks of %d pixels", s, b.blocks, b.pixels);
    check_runs(b.npix, b.pixels, b.blocks, false, "bias blocks");
    const size_t bytes = (size_t)b.blocks * b.cout * 8;
    if (bytes > bpart) bpart = bytes;
    // the forward's and the data gradients' channel tiles
    check_runs(kNkCout[s], kGradTile, grad_tiles(kNkCout[s]), true, "Cout tiles");
    check_runs(kNkUp[s], kGradTile, grad_tiles(kNkUp[s]), true, "up tiles");
    check_runs(kNkSkip[s], kGradTile, grad_tiles(kNkSkip[s]), true, "skip tiles");
    EXPECT(kNkUp[s] % kGradStep == 0 && kNkSkip[s] % kGradStep == 0 && kNkCout[s] % kGradStep == 0, "K steps");
  }
  const size_t goff[7] = {p.off_du3, p.off_dz2, p.off_du2, p.off_dz1, p.off_dl, p.off_part, p.off_bpart};
  const size_t glen[7] = {(size_t)p.npix[3] * 128 * 4, (size_t)p.npix[2] * 128 * 4, (size_t)p.npix[2] * 256 * 4,
                          (size_t)p.npix[1] * 256 * 4, (size_t)p.npix[0] * 256 * 4, part, bpart};
  check_regions(goff, glen, 7, p.total, "grad workspace");
  const size_t foff[3] = {f.off_up, f.off_z1, f.off_z2};
  const size_t flen[3] = {(size_t)f.npix[1] * 512 * 4, (size_t)f.npix[1] * 256 * 4, (size_t)f.npix[2] * 128 * 4};
  check_regions(foff, flen, 3, f.total, "forward workspace");
}

int main() {
  const int mcps[5] = {0, 1, 7, 64, 5000};
  for (int B = 1; B <= 3; ++B)
    for (int h4 = 1; h4 <= 9; ++h4)
      for (int w4 = 1; w4 <= 9; ++w4)
        for (int m : mcps) check_plan(B, h4, w4, m);
  check_plan(1, 19, 19, 0);
  check_plan(16, 19, 19, 0);
  check_plan(16, 19, 19, 482);

  // Known answer 1, by hand: B 2, 2 x 3, chunks of 7.  Pixels 12, 48, 192, 768.  dW1a: 12 pixels, 2 chunks; dW1b: 48,
  // 7 chunks (the last of 6); dW2: 192, 28 chunks (the last of 3); dW3: 768, 110 chunks (the last of 5).  Partials
  // 2 * 256 * 512 * 4 = 1048576, 7 * 256 * 256 * 4 = 1835008, 28 * 128 * 384 * 4 = 5505024, 110 * 64 * 192 * 4 = 5406720:
  // the region takes 5505024.  Bias blocks of 64 pixels: 1, 3, 12 blocks; 2048, 3072, 6144 bytes: 6144.  Regions:
  // d_u3 768 * 128 * 4 = 393216, dZ2 192 * 128 * 4 = 98304, d_u2 196608, dZ1 48 * 256 * 4 = 49152, dL 12288, all
  // multiples of 256.
  NeckGradPlan p;
  EXPECT(neck_grad_plan(2, 2, 3, 7, &p), "known answer 1 refused");
  EXPECT(p.wg[0].Kc == 7 && p.wg[0].chunks == 2 && p.wg[1].chunks == 7 && p.wg[2].chunks == 28 && p.wg[3].chunks == 110,
         "known answer 1 chunks");
  const GradRange c6 = grad_chunk_at(6, 48, 7), c109 = grad_chunk_at(109, 768, 7);
  EXPECT(c6.first == 42 && c6.count == 6 && c109.first == 763 && c109.count == 5, "known answer 1 last chunks");
  EXPECT(p.bs[0].blocks == 1 && p.bs[1].blocks == 3 && p.bs[2].blocks == 12 && p.bs[2].pixels == 64, "known answer 1 bias");
  EXPECT(p.off_du3 == 0 && p.off_dz2 == 393216 && p.off_du2 == 491520 && p.off_dz1 == 688128 && p.off_dl == 737280 &&
             p.off_part == 749568 && p.off_bpart == 6254592 && p.total == 6260736,
         "known answer 1 regions (%zu %zu %zu %zu %zu %zu %zu)", p.off_dz2, p.off_du2, p.off_dz1, p.off_dl, p.off_part,
         p.off_bpart, p.total);
  NeckForwardPlan f;
  EXPECT(neck_forward_plan(2, 2, 3, &f) && f.off_up == 0 && f.off_z1 == 98304 && f.off_z2 == 147456 && f.total == 245760,
         "known answer 1 forward regions");
  // Known answer 2: 16 frames of 608 x 608 (h4 = w4 = 19), the plan's own chunks of 2048.  Pixels 5776, 23104, 92416,
  // 369664: 3, 12 (the last of 576), 46 (the last of 256) and 181 (the last of 1024) chunks; bias blocks of
  // ceil(23104 / 256) = 91 pixels (254 blocks), 361 (256 blocks), 1444 (256 blocks); 5776 pixels are 91 tiles, the
  // last of 16.
  EXPECT(neck_grad_plan(16, 19, 19, 0, &p), "known answer 2 refused");
  EXPECT(p.npix[0] == 5776 && p.npix[3] == 369664 && p.wg[0].chunks == 3 && p.wg[1].chunks == 12 && p.wg[2].chunks == 46 &&
             p.wg[3].chunks == 181 && p.wg[3].Kc == 2048,
         "known answer 2 chunks");
  const GradRange k11 = grad_chunk_at(11, 23104, 2048), k180 = grad_chunk_at(180, 369664, 2048);
  EXPECT(k11.first == 22528 && k11.count == 576 && k180.first == 368640 && k180.count == 1024, "known answer 2 last chunks");
  EXPECT(p.bs[0].pixels == 91 && p.bs[0].blocks == 254 && p.bs[1].pixels == 361 && p.bs[1].blocks == 256 &&
             p.bs[2].pixels == 1444 && p.bs[2].blocks == 256,
         "known answer 2 bias");
  const GradRange t90 = grad_tile_at(90, 5776);
  EXPECT(grad_tiles(5776) == 91 && t90.first == 5760 && t90.count == 16, "known answer 2 tiles");
  // refused
  EXPECT(!neck_grad_plan(0, 4, 4, 0, &p) && !neck_grad_plan(1, 0, 4, 0, &p) && !neck_grad_plan(1, 4, -1, 0, &p) &&
             !neck_grad_plan(1, 4, 4, -1, &p) && !neck_grad_plan(64, 64, 64, 0, &p) && !neck_grad_plan(1, 8192, 1, 0, &p) &&
             !neck_grad_plan(1, 256, 256, 0, &p) && neck_grad_plan(1, 8191, 8, 0, &p) && !neck_forward_plan(0, 1, 1, &f) &&
             !neck_forward_plan(1, 256, 256, &f) && neck_forward_plan(1, 255, 256, &f),
         "refusals");
  std::printf("%ld plans, %ld bad\n", plans, bad);
  return bad ? 1 : 0;
}
