// Host-side plans of the convolution launchers (conv_*_kernel.h, deconv_h3_kernel.h, stem_patch_kernel.h,
// fpn_kernel.h, conv.hip): every check the kernels assume and never make themselves, the grid of a
// launch, the dispatch predicates of conv.hip and the patch stem's frame chunks. Plain C++ (no HIP
// include); a tile's compile-time numbers and a kernel's option bits arrive as plain parameters, so
// tools/conv_plan_check.cpp walks all of it on the CPU. set_error is only declared here.
#pragma once

#include <algorithm>

#include "conv_args.h"
#include "conv_wimage.h"

namespace sfa {

void set_error(const char* fmt, ...);

// ---- the common pieces (fam: the kernel family's name in the message)

inline int ksplit_of(const ConvArgs& a) { return a.ksplit > 1 ? a.ksplit : 1; }

inline bool tile_aligned(const ConvArgs& a, int BK, int BN) {
  return a.Kpad % BK == 0 && (a.nseg != 2 || a.kseg1 % BK == 0) && a.N % BN == 0;
}

inline int check_tiles(const char* fam, const ConvArgs& a, bool have_w, int BK, int BN) {
  if (have_w && tile_aligned(a, BK, BN)) return SFA_OK;
  set_error("%s: K/N not aligned to the tile or no split weights (Kpad=%d kseg1=%d N=%d)", fam, a.Kpad, a.kseg1,
            a.N);
  return SFA_E_UNSUPPORTED;
}

// the split weights, `terms` terms of N rows of `row` 2-byte values, are read with 32-bit offsets
inline int weight_row(const ConvArgs& a) { return a.wstride ? a.wstride : a.Kpad; }
inline int check_weight_bytes(const char* fam, int terms, int N, int row, const char* what = "split weights") {
  if ((unsigned long long)terms * N * row * 2ull < (1ull << 31)) return SFA_OK;
  set_error("%s: %s >= 2 GiB", fam, what);
  return SFA_E_UNSUPPORTED;
}

// a K-slice [wk0, wk0 + K) of wider packed weight rows (wstride 0: the rows are Kpad wide)
inline bool kslice_ok(const ConvArgs& a, int K) { return !a.wstride || (a.wstride >= a.wk0 + K && a.wk0 % 8 == 0); }
inline int check_kslice(const char* fam, const ConvArgs& a) {
  if (kslice_ok(a, a.Kpad)) return SFA_OK;
  set_error("%s: K slice [%d, %d) outside the weight rows (stride %d)", fam, a.wk0, a.wk0 + a.Kpad, a.wstride);
  return SFA_E_INVALID;
}

// split-K of a K cut in k_units units (klabel = kval: what the message names)
inline int check_splitk(const char* fam, const ConvArgs& a, int epi, int k_units, const char* klabel, int kval) {
  const int ks = ksplit_of(a);
  if (ks == 1 || (epi == EPI_STD && k_units % ks == 0 && a.part && (size_t)ks * a.M * a.N <= a.part_floats &&
                  a.N % 4 == 0))
    return SFA_OK;
  set_error("%s: split-K %d unsupported here (%s=%d N=%d)", fam, ks, klabel, kval, a.N);
  return SFA_E_UNSUPPORTED;
}

// mult blocks (split-K slices, deconv phases) per BM x BN output tile
inline int check_grid(const char* fam, int M, int N, int BM, int BN, int mult, unsigned* grid) {
  const long long nblocks = ((long long)M + BM - 1) / BM * (N / BN) * mult;  // 64-bit: M + BM may pass 2^31
  if (nblocks <= 0 || nblocks > 0x7fffffffll) {
    set_error("%s: bad grid (M=%d N=%d)", fam, M, N);
    return SFA_E_INVALID;
  }
  *grid = (unsigned)nblocks;
  return SFA_OK;
}

// ---- launch_conv's shape checks: the kernels assume these and never bounds-check them

inline bool conv_sliced(const ConvArgs& a) { return a.wstride || a.wk0 || a.res_up; }

inline int conv_shape_check(const ConvArgs& a, int epilogue, int math) {
  if (a.N <= 0 || a.N % 64 != 0 || a.M <= 0 || a.Kpad <= 0 || a.Kpad % 16 != 0) {
    set_error("conv: unsupported shape M=%d N=%d Kpad=%d", a.M, a.N, a.Kpad);
    return SFA_E_UNSUPPORTED;
  }
  for (int s = 0; s < a.nseg; ++s) {
    const ConvSeg& g = a.seg[s];
    if (!g.x || g.C < 4 || (g.C & (g.C - 1)) || (1 << g.logC) != g.C || g.KW <= 0 || g.KH <= 0) {
      set_error("conv: bad segment %d (C=%d)", s, g.C);
      return SFA_E_UNSUPPORTED;
    }
    if (g.bytes == 0 || g.bytes >= (1u << 31)) {
      set_error("conv: segment %d input is empty or >= 2 GiB (32-bit buffer offsets)", s);
      return SFA_E_UNSUPPORTED;
    }
    if (g.C < 16 && s != a.nseg - 1) {
      set_error("conv: narrow-channel segment must be last");
      return SFA_E_UNSUPPORTED;
    }
  }
  if (a.nseg == 2 && (a.kseg1 % 16 != 0 || a.kseg1 <= 0 || a.kseg1 >= a.Kpad)) {
    set_error("conv: bad kseg1 %d", a.kseg1);
    return SFA_E_UNSUPPORTED;
  }
  if (conv_sliced(a)) {  // K-sliced weights / half-res residual: conv_h3_kernel only
    if (math != SFA_MATH_FP16X3 || epilogue != EPI_STD) {
      set_error("conv: K-sliced weights / upsampled residual need fp16x3 and the standard epilogue");
      return SFA_E_UNSUPPORTED;
    }
    if (a.res_up && (a.OH % 2 || a.OW % 2 || a.res)) {
      set_error("conv: upsampled residual needs even output dims and no full-res residual");
      return SFA_E_UNSUPPORTED;
    }
  }
  return SFA_OK;
}

// ---- conv.hip's dispatch predicates

// Tile choices are priced at the bench batch (16 frames of the launch's geometry), never at
// a.M: different kernels sum in different orders, so a choice by the batch's row count would
// let a frame's result depend on the batch it is computed in (tests/test_gpu_model.py
// test_batch_invariance_608 holds every path to bit-identical frames across batches).
inline long long tile_rows(const ConvArgs& a) { return 16LL * a.OH * a.OW; }

// Split-K slices of a 128 x 128-tiled body conv (fp16x3, standard epilogue with bias): 2 for the
// 512-wide (layer4) convs, whose 184 output tiles cannot fill 256 CUs (-13..16 %), combined by
// splitk_reduce_kernel. Chosen from the conv width only, so a frame's arithmetic never depends
// on its batch. (Balanced split counts with the slices combined in the kernel were measured 35 %
// slower: tools/experiments/r03, profiles/r03e_ab_splitk_inkernel.txt.)
inline int pick_ksplit(const ConvArgs& a) {
  if (!a.part || !a.bias || conv_sliced(a)) return 1;
  return a.N >= 512 ? 2 : 1;
}

// One-segment 3x3 / stride 1 / pad 1 conv with 32-channel chunks: conv_h3s_kernel applies.
inline bool strip_ok(const ConvArgs& a) {
  const ConvSeg& g = a.seg[0];
  return a.nseg == 1 && g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 && g.C >= 32 &&
         (g.C & 31) == 0 && a.Kpad == 9 * g.C && a.OH == g.H && a.OW == g.W;
}

// The rule table of the fp16 body convs (conv.hip launch_conv_h past its head and FPN rules): the instance
// a conv is given first, BM x BN tiles and the split-K slices. launch_conv_h switches on it; what an
// instance's own check still refuses (partials that do not fit, a K that is no multiple of the K tile)
// falls through there to the conv_h3 forms and on to conv_x6g. tools/conv_plan_check.cpp walks it over the
// model's sixteen residual-layer convs at every input size up to 2048 x 2048.
enum BodyRule {
  BODY_NONE = 0,           // no fp16 body instance: the caller's next family
  BODY_STRIP_128x64,       // conv_h3s, the 64-wide convs (layer1)
  BODY_STRIP_64x128,       // conv_h3s, the 256-wide convs below 3125 pixels a frame (layer3)
  BODY_STRIP_128x64_KS2,   // conv_h3s, the 512-wide convs below 3125 pixels, 2 slices (layer4)
  BODY_STRIP_128x128,      // conv_h3s, every other 128-column conv (layer2; layer3 from 3125 pixels)
  BODY_STRIP_128x128_KS2,  // ... with 2 slices (layer4 from 3125 pixels)
  BODY_R3,                 // conv_r3 128 x 128, R3_BODY: stride-2 / two-segment convs from 3125 pixels
  BODY_R3_KS2,             // ... with 2 slices
  BODY_H3_256x64,          // conv_h3, 64-wide convs that are no strip (or frames under 128 rows)
  BODY_H3_128x64,          // conv_h3 on 16-wide K tiles, 64-wide convs of K < 256 (fp16x3 only)
  BODY_H3_128x128,         // conv_h3, the 128-column convs no rule above takes
  BODY_H3_128x128_KS2,     // ... with 2 slices
  BODY_RULE_COUNT
};

inline const char* body_rule_name(BodyRule r) {
  static const char* const names[BODY_RULE_COUNT] = {
      "none",   "strip_128x64", "strip_64x128", "strip_128x64_ks2", "strip_128x128", "strip_128x128_ks2",
      "r3_body", "r3_body_ks2", "h3_256x64",    "h3_128x64",        "h3_128x128",    "h3_128x128_ks2"};
  return r >= 0 && r < BODY_RULE_COUNT ? names[r] : "?";
}

// terms: 2 is fp16x3, 1 the one-product mode (SFA_MATH_FP16), which has no sliced and no 16-wide-K form.
// The strip kernel wants frames of >= 128 rows (h3s_min_frame_rows), whatever its tile.
inline BodyRule body_conv_rule(const ConvArgs& a, int terms) {
  const bool sliced = conv_sliced(a);
  if (!a.wh || !a.winv || (terms == 1 && sliced)) return BODY_NONE;
  const bool strip = strip_ok(a) && !sliced && a.OH * a.OW >= 128;
  if (a.N == 64) {
    if (strip) return BODY_STRIP_128x64;
    if (a.Kpad >= 256) return BODY_H3_256x64;
    return terms == 2 ? BODY_H3_128x64 : BODY_NONE;
  }
  if (a.N % 128 != 0) return BODY_NONE;
  const int ks = pick_ksplit(a);
  const bool big = tile_rows(a) >= 50000;
  if (strip) {
    if (ks == 1 && a.N == 256 && !big) return BODY_STRIP_64x128;
    if (ks == 2 && a.N == 512 && !big) return BODY_STRIP_128x64_KS2;
    if ((3 * (a.seg[0].C >> 5)) % ks == 0) return ks > 1 ? BODY_STRIP_128x128_KS2 : BODY_STRIP_128x128;
  } else if (big) {
    return ks > 1 ? BODY_R3_KS2 : BODY_R3;
  }
  return ks > 1 && (a.Kpad / 32) % ks == 0 ? BODY_H3_128x128_KS2 : BODY_H3_128x128;
}

// The tile width of the strip instance the rule gives this fp16x3 conv, or 0 when the conv takes another
// family. The model asks it before it hands a launch the conv's W image, which is built for one tile
// width; the launch check (conv_h3s_image_check) refuses an image of another width.
inline int strip_tile_bn(const ConvArgs& a) {
  const BodyRule r = body_conv_rule(a, 2);
  return r == BODY_STRIP_128x64 || r == BODY_STRIP_128x64_KS2 ? 64 : r >= BODY_STRIP_64x128 && r <= BODY_STRIP_128x128_KS2 ? 128 : 0;
}

// ---- the per-family checks: SFA_OK with the launch's grid, or the refusal

inline int conv_f32_check(const ConvArgs& a, int BM, int BN, int BK, unsigned* grid) {
  if (!tile_aligned(a, BK, BN)) {
    set_error("conv: K/N not aligned to the tile (Kpad=%d kseg1=%d N=%d, BK=%d BN=%d)", a.Kpad, a.kseg1, a.N, BK,
              BN);
    return SFA_E_UNSUPPORTED;
  }
  return check_grid("conv", a.M, a.N, BM, BN, 1, grid);
}

// conv_x6 (bf16x6, have_w: a.wx) and conv_x6g (bf16x6, or the fp16x3 form on a.wh / a.winv)
inline int conv_x6_check(const char* fam, const ConvArgs& a, bool have_w, int BM, int BN, int BK, unsigned* grid) {
  if (int rc = check_tiles(fam, a, have_w, BK, BN)) return rc;
  if (int rc = check_weight_bytes(fam, 3, a.N, a.Kpad)) return rc;
  return check_grid(fam, a.M, a.N, BM, BN, 1, grid);
}

inline int conv_h3_check(const ConvArgs& a, int BM, int BN, int BK, int epi, int terms, unsigned* grid) {
  if (int rc = check_tiles("conv_h3", a, a.wh && a.winv, BK, BN)) return rc;
  if (int rc = check_kslice("conv_h3", a)) return rc;
  if (int rc = check_weight_bytes("conv_h3", 2, a.N, weight_row(a))) return rc;
  if (int rc = check_splitk("conv_h3", a, epi, a.Kpad / BK, "Kpad", a.Kpad)) return rc;
  if (int rc = check_grid("conv_h3", a.M, a.N, BM, BN, ksplit_of(a), grid)) return rc;
  if (a.res_up && (a.nseg != 1 || terms != 2)) {  // the upsampled-residual epilogue: one segment, fp16x3
    set_error("conv_h3: upsampled residual with two K-segments or the one-product form");
    return SFA_E_UNSUPPORTED;
  }
  return SFA_OK;
}

// The pre-split strip (presplit) knows two fp16x3 scales per block, those of the frames of its first
// row and the next one, while the epilogue scales every row back by its own frame's: a block must not
// reach a third frame. With frames of at least BM rows none does. The bound is the largest product
// tile's (128 rows) for every tile shape, so which kernel a map takes, and with it a frame's bits,
// depends on the map's size alone, never on the batch; smaller maps take the caller's next kernel,
// which looks every row's frame up. (Frames of equal binary exponent hid this: a 2^9 x brighter third
// frame was split with its neighbour's scale, overflowed fp16 and came out as zeros after the ReLU.)
inline int h3s_min_frame_rows(int BM) { return BM > 128 ? BM : 128; }

inline int conv_h3s_check(const ConvArgs& a, int BM, int BN, int epi, unsigned* grid) {
  const ConvSeg& g = a.seg[0];
  if (!a.wh || !a.winv || !strip_ok(a) || a.N % BN != 0) {
    set_error("conv_h3s: not a one-segment 3x3/s1/p1 conv with C %% 32 == 0 (C=%d Kpad=%d N=%d)", g.C, a.Kpad,
              a.N);
    return SFA_E_UNSUPPORTED;
  }
  if (conv_sliced(a)) {  // the kernel reads none of them
    set_error("conv_h3s: K-sliced weights / upsampled residual are not supported");
    return SFA_E_UNSUPPORTED;
  }
  if (a.OH * a.OW < h3s_min_frame_rows(BM)) {
    set_error("conv_h3s: frames of %d rows are shorter than %d", a.OH * a.OW, h3s_min_frame_rows(BM));
    return SFA_E_UNSUPPORTED;
  }
  if (int rc = check_splitk("conv_h3s", a, epi, 3 * (g.C >> 5), "C", g.C)) return rc;
  if (int rc = check_weight_bytes("conv_h3s", 2, a.N, a.Kpad)) return rc;
  return check_grid("conv_h3s", a.M, a.N, BM, BN, ksplit_of(a), grid);
}

// The image of a conv_h3s instance with h3sopt::W_IMAGE: the whole conv in the strip K order at the
// instance's tile width (after conv_h3s_check: a one-segment 3x3 conv, no K-slice).
inline WImageGeom conv_h3s_image_geom(const ConvArgs& a, int BN) {
  return WImageGeom{a.N, a.Kpad, a.Kpad, 0, BN, 2, 0, a.seg[0].C, 1};
}
inline int conv_h3s_image_check(const ConvArgs& a, int BN) {
  const WImageGeom g = conv_h3s_image_geom(a, BN);
  const char* err = wimage_check(g);
  if (!err && (!a.wimg || a.wimg_bytes != wimage_bytes(g) || a.wimg_bn != BN))
    err = "conv_h3s: W image does not fit this kernel instance";
  if (!err) return SFA_OK;
  set_error("%s", err);
  return SFA_E_INVALID;
}

// conv_r3: res_up_epi / scalar_taps / chunk_major are the instance's r3opt bits of those names
inline int conv_r3_check(const ConvArgs& a, int BM, int BN, int epi, bool res_up_epi, bool scalar_taps,
                         bool chunk_major, unsigned* grid) {
  if (!a.wh || !a.winv || !tile_aligned(a, 32, BN) || (a.res_up && (!res_up_epi || a.res || a.nseg != 1))) {
    set_error("conv_r3: K/N not aligned to the tile, no split weights or an upsampled residual (Kpad=%d kseg1=%d N=%d)", a.Kpad,
              a.kseg1, a.N);
    return SFA_E_UNSUPPORTED;
  }
  if (scalar_taps && (a.nseg != 1 || a.seg[0].C < 32 || a.seg[0].taps > 32)) {
    set_error("conv_r3: fast A addressing needs one segment with C >= 32 (C=%d)", a.seg[0].C);
    return SFA_E_UNSUPPORTED;
  }
  if (chunk_major && (a.seg[0].taps != 9 || a.seg[0].C % 32 != 0 ||
                      (a.nseg == 2 ? a.kseg1 : a.Kpad) != 9 * a.seg[0].C || a.Kpad / 32 > 3600 || a.wstride || a.wk0)) {
    set_error("conv_r3: chunk-major K order needs a 3x3 first segment with C %% 32 == 0 (C=%d Kpad=%d)", a.seg[0].C,
              a.Kpad);
    return SFA_E_UNSUPPORTED;
  }
  for (int s = 0; s < a.nseg; ++s)
    if (a.seg[s].C < 8) {  // a lane's 8 k values must be 8 channels of one input pixel
      set_error("conv_r3: segment %d has C=%d < 8", s, a.seg[s].C);
      return SFA_E_UNSUPPORTED;
    }
  if (int rc = check_kslice("conv_r3", a)) return rc;
  if (int rc = check_weight_bytes("conv_r3", 2, a.N, weight_row(a))) return rc;
  if (int rc = check_splitk("conv_r3", a, epi, a.Kpad / 32, "Kpad", a.Kpad)) return rc;
  return check_grid("conv_r3", a.M, a.N, BM, BN, ksplit_of(a), grid);
}

inline int deconv_check(const DeconvArgs& a, int B, int BM, int BN, unsigned* grid) {
  if (!a.x || !a.wh || !a.winv || !a.bias || !a.y || B < 1 || a.H < 1 || a.W < 1) {
    set_error("deconv: null argument or empty input");
    return SFA_E_INVALID;
  }
  if (a.C < 32 || (a.C & (a.C - 1)) || (1 << a.logC) != a.C || a.K != 4 * a.C || a.N % BN != 0 || a.N <= 0) {
    set_error("deconv: unsupported shape C=%d N=%d K=%d", a.C, a.N, a.K);
    return SFA_E_UNSUPPORTED;
  }
  const unsigned long long in_bytes = (unsigned long long)B * a.H * a.W * a.C * 4ull;
  const unsigned long long out_elems = (unsigned long long)B * a.H * a.W * 4ull * a.N;
  if (in_bytes >= (1ull << 31) || in_bytes != a.bytes || (unsigned long long)a.M != (unsigned long long)B * a.H * a.W ||
      out_elems >= (1ull << 40) || a.H >= 16384 || a.W >= 16384) {
    set_error("deconv: input (%d, %d, %d, %d) is >= 2 GiB (32-bit buffer offsets) or inconsistent", B, a.H, a.W, a.C);
    return SFA_E_UNSUPPORTED;
  }
  if (int rc = check_weight_bytes("deconv", 4, a.N, a.K)) return rc;
  return check_grid("deconv", a.M, a.N, BM, BN, 4, grid);  // the four output parities
}

// The FPN 1x1 convs on the persistent kernels (fpn_kernel.h): one segment, 1x1 / stride 1, K = its
// channel count, NB-wide column tiles, optionally a K-slice of wider weight rows; no split-K.
inline bool fpn_1x1_ok(const ConvArgs& a, int K, int NB) {
  const ConvSeg& g = a.seg[0];
  return a.nseg == 1 && g.KH == 1 && g.KW == 1 && g.stride == 1 && g.pad == 0 && g.C == K && a.Kpad == K &&
         a.N % NB == 0 && a.wh && a.winv && !a.res && a.ksplit <= 1 && a.OH == g.H && a.OW == g.W && kslice_ok(a, K);
}
// ... with the half-resolution residual added upsampled: even output dims
inline bool fpn_skip_ok(const ConvArgs& a, int K, int NB) {
  return fpn_1x1_ok(a, K, NB) && a.res_up && a.OH % 2 == 0 && a.OW % 2 == 0;
}
// `frames` frames of `floats` floats are read through one 32-bit buffer resource
inline bool frames_fit(int frames, size_t floats) { return (size_t)frames * floats * 4 < (1ull << 31); }

// ---- the patch stem (stem_patch_kernel.h)

// Needs the stem's fp16x3 split weights (Kpad >= 196), the input as a.stem_in says (seg 0 describes
// it as 4 channels), a conv output divisible into 16 x 16 tiles, and the side buffer for the pooled
// tile-border parts: 17 rows of 64 floats per tile.
inline int stem_patch_check(const ConvArgs& a) {
  const ConvSeg& g = a.seg[0];
  const bool shape = a.wh && a.winv && a.nseg == 1 && a.N == 64 && g.C == 4 && g.KH == 7 && g.KW == 7 &&
                     g.stride == 2 && g.pad == 3 && a.Kpad >= 196 && a.OH > 0 && a.OW > 0 && a.OH % 16 == 0 &&
                     a.OW % 16 == 0 && a.OH * 2 == g.H && a.OW * 2 == g.W && !a.res && a.relu;
  if (shape && !a.part) {
    set_error("stem_patch: the pooled tile-border parts need the side buffer (a.part)");
    return SFA_E_INVALID;
  }
  if (!shape || a.part_floats < (size_t)a.M / 256 * 17 * 64) {
    set_error("stem_patch: unsupported stem (C=%d k=%d OH=%d OW=%d)", g.C, g.KH, a.OH, a.OW);
    return SFA_E_UNSUPPORTED;
  }
  return SFA_OK;
}

// The kernel reads the input through a buffer resource with 32-bit offsets: batches whose input
// reaches 2 GiB run in frame chunks (the side-buffer slots keep their global tile index).
struct StemChunks {
  int frames, per_chunk, tiles_per_frame;
  size_t frame_bytes;
  int count() const { return ceil_div(frames, per_chunk); }
};
struct StemChunk {
  int f0, frames, tiles;
  size_t x_floats, x_bytes;   // the chunk's input: offset (floats) and size (bytes, < 2^31)
  size_t y_floats, part_floats;  // offsets of its pooled output and of its side-buffer slots
};

// in_channels: 4 (STEM_IN_NHWC4) or 3 (the NCHW3 layouts)
inline int stem_chunk_plan(int frames, int in_channels, int H, int W, StemChunks* p) {
  p->frames = frames;
  p->frame_bytes = (size_t)in_channels * H * W * 4;
  p->tiles_per_frame = (H / 32) * (W / 32);
  p->per_chunk = (int)std::min<size_t>((size_t)frames, ((1ull << 31) - 1) / p->frame_bytes);
  if (p->per_chunk < 1) {
    set_error("stem_patch: one %d x %d frame exceeds the 32-bit buffer offsets", H, W);
    return SFA_E_UNSUPPORTED;
  }
  return SFA_OK;
}

inline StemChunk stem_chunk(const StemChunks& p, int i, int H, int W) {
  StemChunk c;
  c.f0 = i * p.per_chunk;
  c.frames = std::min(p.per_chunk, p.frames - c.f0);
  c.tiles = c.frames * p.tiles_per_frame;
  c.x_floats = (size_t)c.f0 * (p.frame_bytes / 4);
  c.x_bytes = (size_t)c.frames * p.frame_bytes;
  c.y_floats = (size_t)c.f0 * (H / 4) * (W / 4) * 64;
  c.part_floats = (size_t)c.f0 * p.tiles_per_frame * 17 * 64;
  return c;
}

}  // namespace sfa
