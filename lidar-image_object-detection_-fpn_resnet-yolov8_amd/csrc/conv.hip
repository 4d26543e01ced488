// Convolution dispatch: picks the kernel (fp16x3, bf16x6 or f32 MFMA) and its tile
// configuration per layer shape (conv_*_kernel.h). tile_rows, pick_ksplit and strip_ok, which the
// rules below ask, are conv_plan.h's.
#include <cstdlib>

#include "conv_kernel.h"
#include "conv_x6_kernel.h"
#include "conv_h3_kernel.h"
#include "conv_h3s_kernel.h"
#include "conv_r3_kernel.h"
#include "deconv_h3_kernel.h"
#include "fpn_kernel.h"
#include "stem_patch_kernel.h"

namespace sfa {

// bf16x6 tiles per shape, from tools/convbench.hip sweeps on MI355X (round 1):
// wide-N tiles amortise the A split; 8-wave LDS-DMA tiles for the big-M layers.
// Returns SFA_E_UNSUPPORTED when no bf16x6 tile fits (the caller falls back to f32).
static int launch_conv_x6(const ConvArgs& a, int epilogue, hipStream_t st) {
  if (!a.wx) return SFA_E_UNSUPPORTED;
  auto ok = [](int rc) { return rc != SFA_E_UNSUPPORTED; };
  int rc = SFA_E_UNSUPPORTED;
  if (epilogue == EPI_HEAD) {
    if (a.N == 320) rc = launch_conv_x6g_cfg<256, 320, 32, EPI_HEAD, 1>(a, st);
    if (!ok(rc)) rc = launch_conv_x6_cfg<128, 64, 32, 64, 32, EPI_HEAD, 2>(a, st);
    if (!ok(rc)) rc = launch_conv_x6g_cfg<256, 64, 32, EPI_HEAD, 1>(a, st);
    return rc;
  }
  if (a.N == 64) return launch_conv_x6g_cfg<256, 64, 32, EPI_STD, 1>(a, st);
  if (a.N % 128 == 0) {
    if (tile_rows(a) >= 50000) rc = launch_conv_x6_cfg<128, 128, 64, 64, 16, EPI_STD, 2>(a, st);
    else if (tile_rows(a) >= 10000) rc = launch_conv_x6g_cfg<128, 128, 32, EPI_STD, 2>(a, st);
    else rc = launch_conv_x6_cfg<64, 128, 32, 64, 32, EPI_STD, 2>(a, st);
    if (!ok(rc)) rc = launch_conv_x6g_cfg<128, 128, 32, EPI_STD, 2>(a, st);
  }
  return rc;
}

// fp16x3 kernels per shape (tools/convbench.hip sweeps). Round 4 keeps only
// the adopted kernels here; every measured-and-rejected variant (the round-2/3 SFA_TUNE bits) is in
// tools/experiments/r03/ with its convbench hook.
//  * heads: conv_r3_kernel 256 x 320 (all 5 heads of a level per tile), half-tile stagger, 3-stage
//    W ring, 3-block W read-ahead, scalar taps, chunk-major K order, packed head epilogue;
//  * 3x3/s1 body convs on maps of >= 128 rows per frame (smaller ones: "the rest" below, see
//    launch_conv_h3s_cfg): conv_h3s_kernel (A staged once per kh as a row strip for the three kw
//    taps), transposed float4 epilogue, v_fma_mix split; 64-wide 128 x 64 at 3 blocks / CU with the
//    pre-split strip and the residual loaded during the last super-step, 128..512-wide 128 x 128
//    (split-K 2 for the 512-wide; the 256-wide layer3 convs on 64 x 128 tiles);
//  * big-M (layer2) stride-2 and conv + downsample convs: conv_r3_kernel 128 x 128 (A in registers,
//    chunk-major K), -25 % on layer2.0.conv1 against conv_h3;
//  * FPN skip convs (half-resolution residual added bilinearly upsampled in the epilogue):
//    conv_r3_kernel, float4 taps;
//  * the rest (layer3/4 stride-2 and conv + downsample, the FPN low-resolution 1x1 convs, the stem
//    without the patch kernel): conv_h3_kernel on 16x16x32 MFMAs.
// The product instances' option sets (bit semantics: r3opt / h3sopt / h3opt beside the kernels).
// The integers are part of the kernels' names, which the recorded profiles are matched by: pinned below.
// conv_r3 body and FPN skip convs: chunk-major K order (heads' HBM traffic 3.5-4.7x lower:
// profiles/r02_convbench_cmaj.txt) / the upsampled-residual epilogue.
constexpr int R3_BODY = r3opt::ALWAYS | r3opt::CHUNK_MAJOR;
constexpr int R3_FPN = r3opt::ALWAYS | r3opt::RES_UP;
// heads: the stagger (-4.6 / -3.1 / -1.0 % per launch on L1 / L2 / L0, bit-identical,
// profiles/r03h_convbench_heads_stagger.txt), the delayed half issuing every W DMA piece of the K loop
// (round 5: -2.2 %, bit-identical, profiles/r05ah_heads_delayed_half_dma.txt)
constexpr int R3_HEAD_STAG = r3opt::ALWAYS | r3opt::PRIO_HALF | r3opt::MIX_SPLIT | r3opt::READ_AHEAD3 |
                             r3opt::SCALAR_TAPS | r3opt::PACKED_HEAD | r3opt::CHUNK_MAJOR | r3opt::STAGGER |
                             r3opt::DELAYED_DMA;
// heads with W from the conv's pre-tiled LDS image (r3opt::W_IMAGE; ConvArgs::wimg set by the model:
// DESIGN.md §25)
constexpr int R3_HEAD_STAG_IMG = R3_HEAD_STAG | r3opt::W_IMAGE;
// strip kernel: the pre-split strip and the residual prefetch on every tile shape (round 5: with the
// one-latency presplit the 128-wide tiles gain from them too, layer2 -4.6 % / -6.5 % with a residual,
// layer3 -1 / -2 %, bit-identical: profiles/r05j_*; the names of the former two forms stay), the strip in
// registers (late round 5: layer1 -2.7 %, layer2 -2.2 %, layer4 -2.8 %, bench +0.6 %, bit-identical,
// profiles/r05bi_*)
constexpr int H3S_64 = h3sopt::ALWAYS | h3sopt::PRESPLIT | h3sopt::RES_PREFETCH | h3sopt::STRIP_REGS;
constexpr int H3S_128 = H3S_64;
// 128 x 128 tiles (layer2): at 3 blocks / CU without the residual prefetch (198 -> 168 VGPRs; the strip in
// registers freed the LDS), 722 tiles in one round of 768 slots: -1.9 %, bit-identical, profiles/r05bj_*
constexpr int H3S_128W = h3sopt::ALWAYS | h3sopt::PRESPLIT | h3sopt::STRIP_REGS;
// conv_h3: the 64-wide instances as they are, the 128-wide ones with a sched_barrier per column block
constexpr int H3_PLAIN = 0;
constexpr int H3_PIPE = h3opt::PIPE;
static_assert(R3_BODY == 526592 && R3_FPN == 35072 && R3_HEAD_STAG == 3766532 && R3_HEAD_STAG_IMG == 7960836,
              "conv_r3 instance names");
static_assert(H3S_64 == 1166 && H3S_128 == 1166 && H3S_128W == 1038, "conv_h3s instance names");
static_assert((H3S_64 | h3sopt::W_IMAGE) == 3214 && (H3S_128W | h3sopt::W_IMAGE) == 3086,
              "conv_h3s image instance names");
static_assert(H3_PLAIN == 0 && H3_PIPE == 2, "conv_h3 instance names");

// FPN 1x1 convs (commuted: the low-resolution W_a . x and the skip conv with the upsampled
// residual) on the persistent weight-resident kernel (fpn_kernel.h), by channel count.
static int launch_fpn(const ConvArgs& a, hipStream_t st) {
  const int C = a.seg[0].C;
  if (a.res_up) {
    if (a.OW <= 2 * fpn_seg::WHMAX) {  // narrow levels: flat pixel steps, the taps from an LDS row ring
      const int rc = C == 128 ? launch_fpn_seg_cfg<128, 1>(a, st) : C == 256 ? launch_fpn_seg_cfg<256, 1>(a, st)
                                                                             : SFA_E_UNSUPPORTED;
      if (rc != SFA_E_UNSUPPORTED) return rc;
    }
    {  // full rows, the bilinear taps from an LDS ring of source rows
      const int rc = launch_fpn_row(a, st);
      if (rc != SFA_E_UNSUPPORTED) return rc;
    }
    if (C == 64 && a.N % 64 == 0) return launch_fpn_gemm_cfg<64, 64, true, 3>(a, st);
    if (C == 128 && a.N % 128 == 0) return launch_fpn_gemm_cfg<128, 128, true, 2>(a, st);
    if (C == 256 && a.N % 128 == 0) return launch_fpn_gemm_cfg<256, 128, true, 1>(a, st);
  } else {
    if (C == 128 && a.N % 64 == 0) return launch_fpn_gemm_cfg<128, 64, false, 4>(a, st);
    if (C == 256 && a.N % 128 == 0) return launch_fpn_gemm_cfg<256, 128, false, 1>(a, st);
    if (C == 512 && a.N % 64 == 0) return launch_fpn_gemm_cfg<512, 64, false, 1>(a, st);
  }
  return SFA_E_UNSUPPORTED;
}

// A strip launch: the instance with W from the conv's pre-tiled LDS image (h3sopt::W_IMAGE) when
// the model set ConvArgs::wimg (fp16x3; the one-product mode keeps row-major W), else the row-major one.
// conv_plan.h strip_tile_bn gives the tile width of the rule's instance (body_conv_rule, which launch_conv_h
// switches on).
template <int BM, int BN, int WM, int OCC, int ABL, int TERMS>
static int launch_strip(const ConvArgs& a, hipStream_t st) {
  if constexpr (TERMS == 2)
    if (a.wimg) return launch_conv_h3s_cfg<BM, BN, WM, EPI_STD, OCC, ABL | h3sopt::W_IMAGE, 2>(a, st);
  return launch_conv_h3s_cfg<BM, BN, WM, EPI_STD, OCC, ABL, TERMS>(a, st);
}

// The fp16 dispatch rules, once for both modes: TERMS = 2 is fp16x3 (two fp16 terms per operand, three
// products per MAC), TERMS = 1 is SFA_MATH_FP16 (one product per MAC) on the TERMS = 1
// instances of the three MFMA-bound kernel families. One rule table, so a shape takes the same tiles, K
// order and split-K slices in both modes. What only fp16x3 has sits under `if constexpr (TERMS == 2)`:
// other head counts and the other conv_x6g fallbacks, K-sliced weights / upsampled residuals (the FPN
// convs stay fp16x3), 16-wide K-tiles. For those the one-product mode returns SFA_E_UNSUPPORTED and
// launch_conv runs the fp16x3 path.
template <int TERMS>
static int launch_conv_h(const ConvArgs& a, int epilogue, hipStream_t st) {
  static_assert(TERMS == 1 || TERMS == 2, "fp16 terms per operand");
  if (!a.wh || !a.winv) return SFA_E_UNSUPPORTED;
  const bool sliced = conv_sliced(a);  // conv_h3_kernel reads these; the others do not
  if (TERMS == 1 && sliced) return SFA_E_UNSUPPORTED;
  auto ok = [](int rc) { return rc != SFA_E_UNSUPPORTED; };
  int rc = SFA_E_UNSUPPORTED;
  if (epilogue == EPI_HEAD) {
    bool image = false;  // fp16x3 with the model's W image (the one-product mode keeps row-major W)
    if constexpr (TERMS == 2) image = a.wimg != nullptr;
    if (a.N == 320)
      rc = image ? launch_conv_r3_cfg<256, 320, 32, EPI_HEAD, 1, 3, R3_HEAD_STAG_IMG>(a, st)
                 : launch_conv_r3_cfg<256, 320, 32, EPI_HEAD, 1, 3, R3_HEAD_STAG, TERMS>(a, st);
    if constexpr (TERMS == 2)
      if (!ok(rc)) rc = launch_conv_x6g_cfg<256, 64, 32, EPI_HEAD, 1, 16, 3, 0, 64, 1>(a, st);  // other head counts
    return rc;
  }
  if constexpr (TERMS == 2) {
    if (a.fpn_gemm && sliced && a.nseg == 1 && a.seg[0].KH == 1 && a.seg[0].KW == 1 && a.seg[0].stride == 1) {
      rc = launch_fpn(a, st);  // the FPN 1x1 convs (commuted)
      if (ok(rc)) return rc;
    }
    if (a.res_up) {  // FPN skip convs of other widths: conv_r3, transposed float4 epilogue, float4 taps
      if (a.N == 64)
        rc = launch_conv_r3_cfg<128, 64, 32, EPI_STD, 4, 2, R3_FPN>(a, st);
      else if (a.N % 128 == 0)
        rc = launch_conv_r3_cfg<128, 128, 32, EPI_STD, 2, 2, R3_FPN>(a, st);
      return rc;
    }
  }
  // the body convs: the first choice is conv_plan.h body_conv_rule's, what its check refuses falls through
  const BodyRule rule = body_conv_rule(a, TERMS);
  if (a.N == 64) {
    if (rule == BODY_STRIP_128x64) rc = launch_strip<128, 64, 32, 3, H3S_64, TERMS>(a, st);
    if (!ok(rc) && a.Kpad >= 256)
      rc = launch_conv_h3_cfg<256, 64, 32, EPI_STD, 1, 32, 2, false, H3_PLAIN, 1, 64, TERMS>(a, st);
    if constexpr (TERMS == 2) {
      if (!ok(rc)) rc = launch_conv_h3_cfg<128, 64, 32, EPI_STD, 2, 16, 3, false, H3_PLAIN>(a, st);
      if (!ok(rc) && !sliced) rc = launch_conv_x6g_cfg<256, 64, 32, EPI_STD, 1, 16, 3, 0, 64, 1>(a, st);
    }
    return rc;
  }
  if (a.N % 128 == 0) {
    ConvArgs b = a;
    b.ksplit = pick_ksplit(a);
    switch (rule) {
      case BODY_STRIP_64x128:
        // layer3 (362 128-row tiles for 512 block slots): 64 x 128 tiles at 3 blocks / CU fill the
        // chip; same per-element K order, so the same bits (tools/convbench4: 97.7 vs 102.0 us,
        // profiles/r04a_convbench4_stem_regw_tiles.txt)
        rc = launch_strip<64, 128, 16, 3, H3S_128, TERMS>(b, st);
        break;
      case BODY_STRIP_128x64_KS2:
        // layer4 (184 128 x 128 tiles x 2 slices for 512 block slots): the 64-wide layer1 form, 128 x 64
        // tiles at 3 blocks / CU (736 blocks for 768 slots); same slices and per-element K order, so the
        // same bits (tools/convbench4: 102.4-105.0 vs 107.4-110.7 us, profiles/r04o_convbench4_layer4_splits.txt)
        rc = launch_strip<128, 64, 32, 3, H3S_64, TERMS>(b, st);
        break;
      case BODY_STRIP_128x128:
      case BODY_STRIP_128x128_KS2:
        rc = launch_strip<128, 128, 32, 3, H3S_128W, TERMS>(b, st);
        break;
      case BODY_R3:
      case BODY_R3_KS2:  // big-M stride-2 / two-segment: A from registers
        // (3 blocks / CU, late round 5: 150-153 VGPRs, 722 tiles in one round; per launch within 1 %, bench
        // +0.9 % with two steps in flight, bit-identical: profiles/r05bp_*)
        rc = launch_conv_r3_cfg<128, 128, 32, EPI_STD, 3, 2, R3_BODY, TERMS>(b, st);
        break;
      default:  // the conv_h3 forms below
        break;
    }
    if (!ok(rc)) {
      b.tile_cnt = nullptr;  // conv_h3: the reduce launch (conv_h3_kernel.h splitk_ticket)
      if ((a.Kpad / 32) % b.ksplit != 0) b.ksplit = 1;  // K not divisible into the slices: no split
      // the FPN low-resolution 1x1 convs left on conv_h3 (level 1's at mask 61): 64 x 128 tiles, 2 x 2 waves,
      // 3 blocks / CU, same K order (late round 5: 23.4 -> 18.0 us, bit-identical, profiles/r05bo_*; the
      // layer3 / 4 convs on the same tiles were slower, r05bn_*)
      if constexpr (TERMS == 2)
        if (sliced && a.seg[0].KH == 1 && a.seg[0].KW == 1)
          rc = launch_conv_h3_cfg<64, 128, 32, EPI_STD, 3, 32, 2, false, H3_PIPE, 1, 64>(b, st);
      if (!ok(rc)) rc = launch_conv_h3_cfg<128, 128, 32, EPI_STD, 2, 32, 2, false, H3_PIPE, 1, 128, TERMS>(b, st);
    }
    if constexpr (TERMS == 2)
      if (!ok(rc) && !sliced) rc = launch_conv_x6g_cfg<128, 128, 32, EPI_STD, 2, 16, 3, 0, 128, 1>(b, st);
  }
  return rc;
}

int launch_conv(const ConvArgs& a, int epilogue, int math, hipStream_t st) {
  if (int rc = conv_shape_check(a, epilogue, math)) return rc;
  if (conv_sliced(a)) return launch_conv_h<2>(a, epilogue, st);  // K-sliced weights / half-res residual
  if (math == SFA_MATH_FP16) {  // never fails where fp16x3 succeeds: shapes without a one-product kernel run fp16x3
    const int rc = launch_conv_h<1>(a, epilogue, st);
    if (rc != SFA_E_UNSUPPORTED) return rc;
    math = SFA_MATH_FP16X3;
  }
  if (math == SFA_MATH_FP16X3) {
    const int rc = launch_conv_h<2>(a, epilogue, st);
    if (rc != SFA_E_UNSUPPORTED) return rc;
  }
  if (math == SFA_MATH_BF16X6 || math == SFA_MATH_FP16X3) {
    const int rc = launch_conv_x6(a, epilogue, st);
    if (rc != SFA_E_UNSUPPORTED) return rc;
  }
  // Tile choice per shape, from tools/convbench.hip sweeps on MI355X (round 1):
  // 32x64 / 32x32 wave tiles at 4 waves per SIMD hide the gather latency best;
  // BK = 32 pays only for the long-K, few-block layer4 shapes; the LDS-DMA ring
  // (GLDS) gains 2-8 % on the heads and layer3, nothing elsewhere.
  if (epilogue == EPI_HEAD) {
    if (a.N / 64 > SFA_MAX_HEADS) {
      set_error("conv: too many heads");
      return SFA_E_UNSUPPORTED;
    }
    return launch_conv_cfg<128, 64, 32, 64, 16, EPI_HEAD, 4, true>(a, st);
  }
  if (a.N == 64) return launch_conv_cfg<128, 64, 32, 64, 16, EPI_STD, 4>(a, st);
  if (a.N % 128 == 0) {
    if ((tile_rows(a) + 127) / 128 * (a.N / 128) >= 512)
      return launch_conv_cfg<128, 128, 64, 64, 16, EPI_STD, 3>(a, st);
    if ((tile_rows(a) + 63) / 64 * (a.N / 128) >= 512)
      return launch_conv_cfg<64, 128, 32, 64, 16, EPI_STD, 4, true>(a, st);
    if (a.Kpad % 32 == 0 && (a.nseg == 1 || a.kseg1 % 32 == 0))
      return launch_conv_cfg<64, 64, 32, 32, 32, EPI_STD, 4>(a, st);
  }
  return launch_conv_cfg<64, 64, 32, 32, 16, EPI_STD, 4>(a, st);
}

int launch_deconv(const DeconvArgs& a, int B, hipStream_t st) { return launch_deconv_h3_cfg(a, B, st); }

int launch_stem_patch(const ConvArgs& a, hipStream_t st) { return launch_stem_patch_pool(a, st); }

}  // namespace sfa
