// Prints every field of the gradient operators' plans (csrc/block_plan.h, block_train_plan.h, neck_plan.h,
// stem_grad_plan.h, heads_grad_plan.h) for the shapes and caps it is asked about, one line of key=value words per
// query, so that a test can reason from what the plans say and not from a restated formula
// (tests/test_grad_regimes_host.py).  Plain C++: no HIP, no GPU; its own main; built with
// -fsanitize=address,undefined by that test.
//
// Queries, one per line on standard input (or in the file named as the only argument):
//   block       layer block B h w cap
//   block_train layer block B h w cap
//   neck        B h4 w4 cap
//   stem        B H W cap
//   heads       B h w Cin heads cap
// A refused query prints "op=... ok=0" after its arguments.  For every run of chunks or blocks, "last" is the count of
// the last one as grad_chunk_at() / heads_grad_chunk() give it: what the kernels call.
#include <cstdio>
#include <cstring>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/block_plan.h"
#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/block_train_plan.h"
#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/heads_grad_plan.h"
#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/neck_plan.h"
#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/stem_grad_plan.h"

using namespace sfa;

static void put_split(const char* pre, const GradSplitK& k) {
  std::printf(" %s.npix=%d %s.Kc=%d %s.chunks=%d %s.last=%d", pre, k.npix, pre, k.Kc, pre, k.chunks, pre,
              grad_chunk_at(k.chunks - 1, k.npix, k.Kc).count);
}

static void put_blocks(const char* pre, const GradBias& b) {
  std::printf(" %s.npix=%d %s.cout=%d %s.pixels=%d %s.blocks=%d %s.last=%d %s.bytes=%zu", pre, b.npix, pre, b.cout, pre,
              b.pixels, pre, b.blocks, pre, grad_chunk_at(b.blocks - 1, b.npix, b.pixels).count, pre, grad_bias_bytes(b));
}

static void put_shape(const BlockShape& s) {
  std::printf(" cin=%d cout=%d stride=%d downsample=%d oh=%d ow=%d npix_in=%d npix_out=%d", s.cin, s.cout, s.stride,
              s.downsample, s.oh, s.ow, s.npix_in, s.npix_out);
}

static void put_wgrads(const BlockWgrad* wg) {
  const char* names[3] = {"wg0", "wg1", "wg2"};
  for (int i = 0; i < 3; ++i) {
    put_split(names[i], wg[i]);
    std::printf(" %s.rows=%d %s.cin=%d %s.taps=%d", names[i], wg[i].rows, names[i], wg[i].cin, names[i], wg[i].taps);
  }
}

static void dump_block(int layer, int block, int B, int h, int w, int cap) {
  std::printf("op=block layer=%d block=%d B=%d h=%d w=%d cap=%d", layer, block, B, h, w, cap);
  BlockGradPlan p;
  if (!block_grad_plan(layer, block, B, h, w, cap, &p)) {
    std::printf(" ok=0\n");
    return;
  }
  std::printf(" ok=1");
  put_shape(p.s);
  put_wgrads(p.wg);
  put_blocks("bs", p.bs);
  std::printf(" off_da=%zu off_part=%zu off_bpart=%zu total=%zu\n", p.off_da, p.off_part, p.off_bpart, p.total);
}

static void dump_block_train(int layer, int block, int B, int h, int w, int cap) {
  std::printf("op=block_train layer=%d block=%d B=%d h=%d w=%d cap=%d", layer, block, B, h, w, cap);
  BlockTrainForwardPlan f;
  BlockTrainGradPlan p;
  if (!block_train_forward_plan(layer, block, B, h, w, cap, &f) || !block_train_grad_plan(layer, block, B, h, w, cap, &p)) {
    std::printf(" ok=0\n");
    return;
  }
  std::printf(" ok=1 nbn=%d", p.nbn);
  put_shape(p.s);
  put_wgrads(p.wg);
  put_blocks("fst", f.st);
  put_blocks("st", p.st);
  std::printf(" f.off_wk0=%zu f.off_wk1=%zu f.off_wk2=%zu f.off_spart=%zu f.off_coef=%zu f.total=%zu", f.off_wk[0],
              f.off_wk[1], f.off_wk[2], f.off_spart, f.off_coef, f.total);
  std::printf(" off_dz2=%zu off_dzd=%zu off_da=%zu off_dz1=%zu off_wt0=%zu off_wt1=%zu off_part=%zu off_rpart=%zu"
              " off_sums=%zu total=%zu\n",
              p.off_dz2, p.off_dzd, p.off_da, p.off_dz1, p.off_wt[0], p.off_wt[1], p.off_part, p.off_rpart, p.off_sums,
              p.total);
}

static void dump_neck(int B, int h4, int w4, int cap) {
  std::printf("op=neck B=%d h4=%d w4=%d cap=%d", B, h4, w4, cap);
  NeckGradPlan p;
  if (!neck_grad_plan(B, h4, w4, cap, &p)) {
    std::printf(" ok=0\n");
    return;
  }
  std::printf(" ok=1 npix0=%d npix1=%d npix2=%d npix3=%d", p.npix[0], p.npix[1], p.npix[2], p.npix[3]);
  const char* wn[4] = {"wg0", "wg1", "wg2", "wg3"};
  const char* bn[3] = {"bs0", "bs1", "bs2"};
  for (int i = 0; i < 4; ++i) {
    put_split(wn[i], p.wg[i]);
    std::printf(" %s.rows=%d %s.cols=%d", wn[i], p.wg[i].rows, wn[i], p.wg[i].cols);
  }
  for (int f = 0; f < 3; ++f) put_blocks(bn[f], p.bs[f]);
  std::printf(" off_du3=%zu off_dz2=%zu off_du2=%zu off_dz1=%zu off_dl=%zu off_part=%zu off_bpart=%zu total=%zu\n", p.off_du3,
              p.off_dz2, p.off_du2, p.off_dz1, p.off_dl, p.off_part, p.off_bpart, p.total);
}

static void dump_stem(int B, int H, int W, int cap) {
  std::printf("op=stem B=%d H=%d W=%d cap=%d", B, H, W, cap);
  StemGradPlan p;
  if (!stem_grad_plan(B, H, W, cap, &p)) {
    std::printf(" ok=0\n");
    return;
  }
  const StemShape& s = p.s;
  std::printf(" ok=1 oh=%d ow=%d ph=%d pw=%d npix_x=%d npix_a=%d npix_p=%d", s.oh, s.ow, s.ph, s.pw, s.npix_x, s.npix_a,
              s.npix_p);
  put_split("wg", p.wg);
  std::printf(" wg.rows=%d wg.cin=%d wg.taps=%d", p.wg.rows, p.wg.cin, p.wg.taps);
  put_blocks("bs", p.bs);
  // the data gradient's launch (sfa_model_stem_grad): passes of kSgDgradPixels image pixels over at most
  // kSgDgradMaxBlocks blocks, block b taking passes b, b + blocks, ...
  const int passes = (s.npix_x + kSgDgradPixels - 1) / kSgDgradPixels;
  const int blocks = passes < kSgDgradMaxBlocks ? passes : kSgDgradMaxBlocks;
  std::printf(" dg.pixels=%d dg.passes=%d dg.blocks=%d dg.last=%d", kSgDgradPixels, passes, blocks,
              grad_chunk_at(passes - 1, s.npix_x, kSgDgradPixels).count);
  std::printf(" off_da=%zu off_part=%zu off_bpart=%zu total=%zu\n", p.off_da, p.off_part, p.off_bpart, p.total);
}

static void dump_heads(int B, int h, int w, int Cin, int heads, int cap) {
  std::printf("op=heads B=%d h=%d w=%d Cin=%d heads=%d cap=%d", B, h, w, Cin, heads, cap);
  HeadsGradPlan p;
  if (!heads_grad_plan(B, h, w, Cin, heads, cap, &p)) {
    std::printf(" ok=0\n");
    return;
  }
  const long long npix = (long long)B * h * w;
  const long long dh_last = npix - (long long)(p.dh_blocks - 1) * p.dh_pixels;
  std::printf(" ok=1 M=%d rows_per_chunk=%d chunks_per_frame=%d num_chunks=%d Kc=%d last_rows=%d dh_pixels=%d dh_blocks=%d"
              " dh_last=%lld dh_slots=%d Na=%d Nb=%d",
              p.M, p.rows_per_chunk, p.chunks_per_frame, p.num_chunks, p.Kc, heads_grad_chunk(p, p.num_chunks - 1).rows,
              p.dh_pixels, p.dh_blocks, dh_last, p.dh_slots, p.Na, p.Nb);
  std::printf(" off_hidden=%zu off_dhidden=%zu off_part=%zu off_dpart=%zu off_terms=%zu off_amax=%zu total=%zu\n", p.off_hidden,
              p.off_dhidden, p.off_part, p.off_dpart, p.off_terms, p.off_amax, p.total);
}

int main(int argc, char** argv) {
  std::FILE* in = stdin;
  if (argc == 2) {
    in = std::fopen(argv[1], "r");
    if (!in) {
      std::fprintf(stderr, "grad_plan_dump: cannot open %s\n", argv[1]);
      return 2;
    }
  } else if (argc > 2) {
    std::fprintf(stderr, "usage: grad_plan_dump [queries.txt]  (else queries on standard input)\n");
    return 2;
  }
  char line[256], op[32];
  long n = 0, unknown = 0;
  while (std::fgets(line, sizeof line, in)) {
    int a[6] = {0, 0, 0, 0, 0, 0};
    const int got = std::sscanf(line, "%31s %d %d %d %d %d %d", op, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
    if (got < 1 || op[0] == '#') continue;
    ++n;
    if (!std::strcmp(op, "block") && got == 7) dump_block(a[0], a[1], a[2], a[3], a[4], a[5]);
    else if (!std::strcmp(op, "block_train") && got == 7) dump_block_train(a[0], a[1], a[2], a[3], a[4], a[5]);
    else if (!std::strcmp(op, "neck") && got == 5) dump_neck(a[0], a[1], a[2], a[3]);
    else if (!std::strcmp(op, "stem") && got == 5) dump_stem(a[0], a[1], a[2], a[3]);
    else if (!std::strcmp(op, "heads") && got == 7) dump_heads(a[0], a[1], a[2], a[3], a[4], a[5]);
    else {
      ++unknown;
      std::printf("op=%s ok=0 unknown=1\n", op);
    }
  }
  if (in != stdin) std::fclose(in);
  std::fprintf(stderr, "grad_plan_dump: %ld queries, %ld unknown\n", n, unknown);
  return unknown ? 1 : 0;
}
