// Host-only check of csrc/block_plan.h (plain C++: no HIP, no GPU): walks the eight blocks at B 1..2, h and w 1..9
// (odd and even, so both strides meet both parities) plus the row widths 66 and 70 that cross a pixel tile, and
// max_chunk_pixels in {0, 1, 3, 17, 5000}, and checks for every plan that the shape is the block's, that the pixel
// tiles of the data gradients and the chunks of the weight and bias gradients partition their ranges (the last run
// short, never empty), that K_c is the largest chunk and within the cap, that every input pixel's nine tap sources
// are exactly the output pixels whose window holds it, and that the workspace regions of both entries are disjoint,
// aligned and inside the reported size; then two plans worked by hand and the refused shapes.  Built with
// -fsanitize=address,undefined by tests/test_block_plan.py.
#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/block_plan.h"
#include "plan_check.h"

using namespace sfa;

// block_tap_source against the forward's own index arithmetic i = o s - 1 + k, along one axis
static void check_taps(int n, int s, int on) {
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      int want = -1;
      for (int o = 0; o < on; ++o)
        if (o * s - 1 + k == i) want = o;
      EXPECT(block_tap_source(i, k, s, on) == want, "tap source i %d k %d s %d on %d", i, k, s, on);
    }
}

static void check_plan(int layer, int block, int B, int h, int w, int mcp) {
  BlockGradPlan p;
  BlockForwardPlan f;
  const bool ok = block_grad_plan(layer, block, B, h, w, mcp, &p) && block_forward_plan(layer, block, B, h, w, &f);
  EXPECT(ok, "refused layer%d.%d B %d h %d w %d mcp %d", layer, block, B, h, w, mcp);
  if (!ok) return;
  ++plans;
  const BlockShape& s = p.s;
  const bool ds = block == 0 && layer > 1;
  EXPECT(s.cout == 64 << (layer - 1) && s.cin == (ds ? s.cout / 2 : s.cout) && s.stride == (ds ? 2 : 1) &&
             s.downsample == (ds ? 1 : 0),
         "shape of layer%d.%d", layer, block);
  EXPECT(s.oh == (h + s.stride - 1) / s.stride && s.ow == (w + s.stride - 1) / s.stride, "output dims");
  EXPECT((s.oh - 1) * s.stride < h && (s.ow - 1) * s.stride < w, "the last output pixel's centre is outside the map");
  EXPECT(s.npix_in == B * h * w && s.npix_out == B * s.oh * s.ow && f.s.npix_out == s.npix_out, "pixel counts");
  check_runs(s.npix_in, kGradTile, grad_tiles(s.npix_in), true, "input pixel tiles");
  check_runs(s.npix_out, kGradTile, grad_tiles(s.npix_out), true, "output pixel tiles");
  check_taps(h, s.stride, s.oh);
  check_taps(w, s.stride, s.ow);
  const int cap = mcp > 0 ? mcp : kGradChunkPixels;
  size_t part = 0;
  for (int i = 0; i < 3; ++i) {
    const BlockWgrad& g = p.wg[i];
    EXPECT(g.rows == s.cout && g.cin == (i == 1 ? s.cout : s.cin) && g.taps == (i == 2 ? (ds ? 1 : 0) : 9), "wgrad %d dims", i);
    EXPECT(g.Kc >= 1 && g.Kc <= cap && g.Kc <= g.npix && g.npix == s.npix_out, "wgrad %d Kc %d", i, g.Kc);
    EXPECT(g.chunks == (g.npix + g.Kc - 1) / g.Kc, "wgrad %d chunks", i);
    EXPECT(g.rows % kGradTile == 0 && g.cin % kGradTile == 0, "wgrad %d channel tiles", i);
    check_runs(g.npix, g.Kc, g.chunks, false, "split-K chunks");
    const size_t bytes = (size_t)g.chunks * g.rows * g.taps * g.cin * 4;
    if (bytes > part) part = bytes;
  }
  EXPECT(p.bs.npix == s.npix_out && p.bs.cout == s.cout && p.bs.pixels >= kGradBiasMinPixels && p.bs.blocks <= kGradBiasMaxBlocks,
         "bias plan");
  check_runs(p.bs.npix, p.bs.pixels, p.bs.blocks, false, "bias blocks");
  const size_t goff[3] = {p.off_da, p.off_part, p.off_bpart};
  const size_t glen[3] = {(size_t)s.npix_out * s.cout * 4, part, (size_t)p.bs.blocks * s.cout * 8};
  check_regions(goff, glen, 3, p.total, "grad workspace");
  const size_t foff[3] = {f.off_amax_x, f.off_amax_mid, f.off_part};
  const size_t flen[3] = {(size_t)B * SFA_AMAX_WORDS * 4, (size_t)B * SFA_AMAX_WORDS * 4, f.part_floats * 4};
  check_regions(foff, flen, 3, f.total, "forward workspace");
  EXPECT(f.part_floats == (s.cout >= 512 ? (size_t)2 * s.npix_out * s.cout : 0), "split-K partials");
}

int main() {
  const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 66, 70};
  const int caps[] = {0, 1, 3, 17, 5000};
  for (int layer = 1; layer <= 4; ++layer)
    for (int block = 0; block < 2; ++block)
      for (int B = 1; B <= 2; ++B)
        for (int h : sizes)
          for (int w : sizes) {
            if (h > 9 && w > 9) continue;
            for (int mcp : caps) check_plan(layer, block, B, h, w, mcp);
          }

  // by hand: layer2.0 at (2, 5, 7) with chunks of at most 17 pixels.  Stride 2: 3 x 4 outputs per frame, 24 output
  // pixels in chunks of 17 and 7; dW1' 128 x 576, dW2' 128 x 1152, dWd' 128 x 64: the partials are 2 x 128 x 1152 x 4
  // = 1,179,648 bytes after dA (24 x 128 x 4 = 12,288 bytes); one bias block of 64 pixels: 128 x 8 = 1,024 bytes.
  {
    BlockGradPlan p;
    EXPECT(block_grad_plan(2, 0, 2, 5, 7, 17, &p), "hand plan 1 refused");
    EXPECT(p.s.cin == 64 && p.s.cout == 128 && p.s.stride == 2 && p.s.oh == 3 && p.s.ow == 4, "hand plan 1 shape");
    EXPECT(p.s.npix_in == 70 && p.s.npix_out == 24, "hand plan 1 pixels");
    EXPECT(p.wg[0].Kc == 17 && p.wg[0].chunks == 2 && p.wg[2].taps == 1 && p.wg[2].cin == 64, "hand plan 1 chunks");
    EXPECT(p.bs.pixels == 64 && p.bs.blocks == 1, "hand plan 1 bias");
    EXPECT(p.off_da == 0 && p.off_part == 12288 && p.off_bpart == 12288 + 1179648 && p.total == 12288 + 1179648 + 1024,
           "hand plan 1 regions %zu %zu %zu", p.off_part, p.off_bpart, p.total);
    EXPECT(grad_tiles(70) == 2 && grad_tile_at(1, 70).first == 64 && grad_tile_at(1, 70).count == 6, "hand plan 1 tiles");
  }
  // by hand: layer4.1 at (16, 19, 19), the plan's own chunks.  5,776 pixels in chunks of 2,048, 2,048 and 1,680; the
  // partials are 3 x 512 x 4,608 x 4 = 28,311,552 bytes after dA (5,776 x 512 x 4 = 11,829,248 bytes); 91 bias blocks
  // of 64 pixels (the last of 16): 91 x 512 x 8 = 372,736 bytes.  Forward: two records of 16 x 1,024 bytes, then the
  // split-K partials 2 x 5,776 x 512 floats.
  {
    BlockGradPlan p;
    BlockForwardPlan f;
    EXPECT(block_grad_plan(4, 1, 16, 19, 19, 0, &p) && block_forward_plan(4, 1, 16, 19, 19, &f), "hand plan 2 refused");
    EXPECT(p.s.cin == 512 && p.s.cout == 512 && p.s.stride == 1 && p.s.npix_out == 5776, "hand plan 2 shape");
    EXPECT(p.wg[1].Kc == 2048 && p.wg[1].chunks == 3 && grad_chunk_at(2, 5776, 2048).count == 1680, "hand plan 2 chunks");
    EXPECT(p.wg[2].taps == 0, "hand plan 2 has no downsample");
    EXPECT(p.bs.pixels == 64 && p.bs.blocks == 91 && grad_chunk_at(90, 5776, 64).count == 16, "hand plan 2 bias");
    EXPECT(p.off_part == 11829248 && p.off_bpart == 11829248 + 28311552 && p.total == 11829248 + 28311552 + 372736,
           "hand plan 2 regions");
    EXPECT(f.off_amax_mid == 16384 && f.off_part == 32768 && f.part_floats == (size_t)2 * 5776 * 512 &&
               f.total == 32768 + (size_t)2 * 5776 * 512 * 4,
           "hand plan 2 forward");
  }
  // refusals
  {
    BlockGradPlan p;
    BlockForwardPlan f;
    EXPECT(!block_grad_plan(0, 0, 1, 4, 4, 0, &p) && !block_grad_plan(5, 0, 1, 4, 4, 0, &p), "layer out of range");
    EXPECT(!block_grad_plan(1, -1, 1, 4, 4, 0, &p) && !block_grad_plan(1, 2, 1, 4, 4, 0, &p), "block out of range");
    EXPECT(!block_grad_plan(1, 0, 0, 4, 4, 0, &p) && !block_grad_plan(1, 0, 1, 0, 4, 0, &p) &&
               !block_grad_plan(1, 0, 1, 4, -3, 0, &p),
           "non-positive sizes");
    EXPECT(!block_grad_plan(1, 0, 1, 4, 4, -1, &p), "negative cap");
    EXPECT(!block_forward_plan(1, 0, 1 << 20, 64, 64, &f) && !block_grad_plan(1, 0, 1 << 20, 64, 64, 0, &p), "2^32 pixels");
    // 64 channels x 4 bytes: 2^23 pixels are 2^31 bytes (refused), one row fewer is not
    EXPECT(!block_grad_plan(1, 0, 1, 2048, 4096, 0, &p) && block_grad_plan(1, 0, 1, 2047, 4096, 0, &p), "the 2^31-byte edge");
    // stride 2: the input is the smaller map in bytes per pixel, the output has twice the channels on a quarter of them
    EXPECT(!block_grad_plan(2, 0, 1, 2048, 4096, 0, &p) && block_grad_plan(2, 0, 1, 2047, 4096, 0, &p), "the edge at stride 2");
  }
  std::printf("%ld plans, %ld bad\n", plans, bad);
  return bad ? 1 : 0;
}
