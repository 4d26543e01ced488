// The convolution launchers' argument structs and their host-side arithmetic: plain C++ (no HIP
// include), so the launch plans (conv_plan.h) and their CPU check (tools/conv_plan_check.cpp) compile
// without a GPU toolchain. conv.h adds the device helpers.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/sfa_hip.h"
#include "host_math.h"

namespace sfa {

// One K-segment of the implicit GEMM: an NHWC input read through a
// KHxKW/stride/pad window.  A conv with a fused 1x1 downsample residual, or an
// FPN 1x1 conv over a channel concat, is two segments concatenated along K.
struct ConvSeg {
  const float* x;
  int H, W, C, logC;   // C is a power of two (4 .. 512)
  int KH, KW, stride, pad;
  int taps;            // KH * KW
  int kdiv_mul, kdiv_sh;  // tap / KW == (tap * kdiv_mul) >> kdiv_sh for tap < 64
  unsigned bytes;      // size of x in bytes (< 2^31): buffer-load range, OOB -> 0
};

// Fills a segment; returns false if the tensor is too large for 32-bit offsets.
inline bool make_seg(ConvSeg& g, const float* x, int B, int H, int W, int C, int k, int stride, int pad) {
  g.x = x;
  g.H = H;
  g.W = W;
  g.C = C;
  g.logC = ilog2(C);
  g.KH = g.KW = k;
  g.stride = stride;
  g.pad = pad;
  g.taps = k * k;
  g.kdiv_mul = 1;
  g.kdiv_sh = 0;
  for (int sh = 0; sh < 16 && k > 1; ++sh) {
    const int mul = ((1 << sh) + k - 1) / k;
    bool ok = true;
    for (int t = 0; t < 64 && ok; ++t) ok = ((t * mul) >> sh) == t / k;
    if (ok) {
      g.kdiv_mul = mul;
      g.kdiv_sh = sh;
      break;
    }
  }
  const unsigned long long bytes = (unsigned long long)B * H * W * C * 4ull;
  g.bytes = (unsigned)bytes;
  return bytes < (1ull << 31);
}

// EPI_POOL (fp16x3 stem): bias + ReLU, then the 3x3/s2/p1 max-pool of the tile in LDS;
// y is the POOLED output (zeroed beforehand), rows of a block = one 16x16 spatial tile.
enum ConvEpilogue { EPI_STD = 0, EPI_HEAD = 1, EPI_POOL = 2 };

// fp16x3 activation scales (SFA_MATH_FP16X3).  max |x| of an activation tensor is kept
// PER FRAME (so a frame's result never depends on the rest of its batch), each in
// SFA_AMAX_WORDS words: SFA_AMAX_SHARDS shards one 128-B line apart, shard = blockIdx & 7
// of the producing workgroup; a reader takes the max over the shards.  Tensor t, frame b
// lives at base_t + b * SFA_AMAX_WORDS.
constexpr int SFA_AMAX_SHARDS = 8;
constexpr int SFA_AMAX_STRIDE = 32;   // words between shards
constexpr int SFA_AMAX_WORDS = SFA_AMAX_SHARDS * SFA_AMAX_STRIDE;

enum StemInput { STEM_IN_NHWC4 = 0, STEM_IN_NCHW3 = 1, STEM_IN_NCHW3_FLIP = 2 };

// n / d for 0 <= n < 2^31 by a multiply-high (round-up method with an add, Granlund-Montgomery):
// q = (umulhi(n, m) + n) >> s, s = ceil(log2 d), m = floor(2^32 (2^s - d) / d) + 1 < 2^32 — exact for
// every d >= 1 and n < 2^31 (the 33-bit magic 2^32 + m >= 2^(32+s) / d with an error below d <= 2^s).
// 3 VALU instead of the ~20 of a generic 32-bit division by a runtime divisor.
struct FastDiv {
  unsigned m;
  int s;
};
inline FastDiv make_fast_div(unsigned d) {
  int s = 0;
  while ((1ull << s) < d) ++s;
  const unsigned long long m = ((1ull << 32) * ((1ull << s) - d)) / d + 1;
  return FastDiv{(unsigned)m, s};
}

struct ConvArgs {
  ConvSeg seg[2];
  int nseg;
  int kseg1;           // first K index of segment 1 (multiple of 16)
  int Kpad;            // total K (multiple of 16)
  const float* w;      // [N][Kpad] (OHWI per segment, K-concatenated, zero padded)
  const uint16_t* wx;  // bf16x6 path: w split into 3 bf16 terms, [3][N][Kpad]
  // fp16x3 path: w[n][k] * 2^e[n] split into 2 fp16 terms, [2][N][Kpad]; winv[n] = 2^-e[n]
  const uint16_t* wh;
  const float* winv;
  // fp16x3 path: per K-segment, the per-frame max |x| words of that segment's input
  // (written by its producer; frame b at + b * SFA_AMAX_WORDS), or null (scale 1)
  const unsigned* amax_in[2];
  unsigned* amax_out;  // this conv's per-frame max |y| is recorded here, or null
  const float* bias;   // [N]
  const float* res;    // residual [M][N] (NHWC) or nullptr
  float* y;            // output [M][N] (NHWC)
  int M, N, OH, OW;
  int relu;
  // EPI_HEAD: block column j = head j (64 channels each); bias+ReLU, then the
  // head's 1x1 conv (64 -> c_j <= 4) with bias, written channel-planar to
  // hout[(hoff[j] + c) * M + m].
  const float* hw1;    // [nheads][4][64]
  const float* hb1;    // [nheads][4]
  int hch[SFA_MAX_HEADS];
  int hoff[SFA_MAX_HEADS];
  float* hout;
  // split-K (EPI_STD, fp16x3): workspace for [ksplit][M][N] partial sums, or null (no
  // split); launch_conv picks ksplit for grids too small to fill the chip, the conv
  // writes scaled partials and a reduce kernel applies the epilogue.
  float* part;
  size_t part_floats;
  int ksplit;
  // fp16x3 (conv_h3_kernel) K-slice of a wider packed conv: the fp16 terms' row stride is
  // wstride (0: Kpad) and the slice starts at K column wk0. Used by the FPN 1x1 convs, which
  // run their two K-segments as two convs at different resolutions (model.hip).
  int wstride, wk0;
  // EPI_STD: residual given at HALF resolution [B][OH/2][OW/2][N], added bilinearly
  // upsampled x2 (align_corners, source step res_sh / res_sw), or null. bias may be null.
  const float* res_up;
  float res_sh, res_sw;
  // Round-3 experiment knobs (tools/experiments/r03 kernels and their convbench hooks only): tune
  // bits, stem ablations. The product kernels never read them and the model leaves them zero.
  int tune;
  int stem_abl;
  // split-K tickets (>= one word per output tile, zeroed before the launch): with them the last slice
  // of a tile combines the partials in the conv kernel (conv_h3_kernel.h splitk_ticket) instead of
  // splitk_reduce_kernel; null: the reduce launch
  unsigned* tile_cnt;
  int tile_cnt_words;  // capacity of tile_cnt (words): a launch with more output tiles takes the reduce launch
  // Patch stem input (stem_patch_kernel.h): STEM_IN_NHWC4 (the voxeliser's layout), STEM_IN_NCHW3
  // (the reference's (B, 3, H, W)), STEM_IN_NCHW3_FLIP (read as torch.flip(x, [2, 3])); every
  // 16 x 16 output tile scales its fp16x3 patch by its own max |x| (no layout / amax pass).
  int stem_in;
  // FPN 1x1 convs: 1 = may run on the persistent weight-resident kernel (fpn_kernel.h), 0 = the
  // per-tile conv_h3 / conv_r3 kernels (model option SFA_OPT_FPN_GEMM)
  int fpn_gemm;
  // multiply-high divisions by the input width / height (filled by the strip kernel's launch) and by
  // the output width / height (conv_r3's)
  FastDiv fd_w, fd_h, fd_ow, fd_oh;
  // fp16x3: the pre-tiled LDS image of wh for the kernel instance this conv runs on (conv_wimage.h:
  // the instance's tile width and K order), wimg_bytes long, or null: the kernels gather their W
  // pieces from the row-major terms. Kernel instances without an image form never read it.
  const unsigned char* wimg;
  unsigned wimg_bytes;
  // the tile width the image was built for (an image's size does not depend on it); read by the strip
  // kernel's launch check, the heads' 256 x 320 instance has one width
  int wimg_bn;
};

// Transposed convolution k=4 / s=2 / p=1 + folded BN + ReLU, fp16x3 (deconv_h3_kernel.h): the four
// output parities as four 2 x 2 convolutions of the input, one launch.
struct DeconvArgs {
  const float* x;          // input NHWC (B, H, W, C), C a power of two, multiple of 32
  int H, W, C, logC;
  unsigned bytes;          // size of x in bytes (< 2^31): buffer-load range, OOB -> 0
  const uint16_t* wh;      // [4 phases][2 terms][N][K] fp16, K = 4 C; phase = 2 py + px
  const float* winv;       // [4][N]
  const float* bias;       // [N]
  const unsigned* amax_in; // per-frame max |x| words of the input (conv.h), or null (scale 1)
  unsigned* amax_out;      // per-frame max |y| words of the output, or null
  float* y;                // output NHWC (B, 2H, 2W, N)
  int M, N, K;             // M = B H W rows per phase
  FastDiv fd_w, fd_h;
};

}  // namespace sfa
