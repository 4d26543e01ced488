// Implicit-GEMM convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32) for gfx950.
#pragma once

#include "common.h"
#include "conv_args.h"

namespace sfa {

__device__ __forceinline__ void amax_atomic(unsigned* amax, int frame, float v) {
  atomicMax(amax + (size_t)frame * SFA_AMAX_WORDS + (blockIdx.x & (SFA_AMAX_SHARDS - 1)) * SFA_AMAX_STRIDE,
            __float_as_uint(v));
}

// Block-wide commit of the maxima of frames fb0 (mx0) and fb0 + 1 (mx1): every thread of
// the block calls it; one no-return atomic per frame and block.  `red` is 2 * NW floats of
// LDS no wave is using (the call synchronises the block).
template <int NW>
__device__ __forceinline__ void amax_commit_block(unsigned* amax, int fb0, float mx0, float mx1,
                                                  float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mx0 = fmaxf(mx0, __shfl_xor(mx0, o, 64));
    mx1 = fmaxf(mx1, __shfl_xor(mx1, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[2 * (threadIdx.x >> 6)] = mx0;
    red[2 * (threadIdx.x >> 6) + 1] = mx1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float m0 = red[0], m1 = red[1];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      m0 = fmaxf(m0, red[2 * w]);
      m1 = fmaxf(m1, red[2 * w + 1]);
    }
    if (m0 > 0.f) amax_atomic(amax, fb0, m0);
    if (m1 > 0.f) amax_atomic(amax, fb0 + 1, m1);  // only rows of a real frame raise it
  }
}

// Scale of frame `frame` for an fp16x3 consumer: 2^(13 - e) for max |x| in [2^e, 2^(e+1))
// over its segments' inputs, so every scaled |x| < 2^14 (4x below the fp16 maximum);
// zero / unset / non-finite max -> 1.  sinv = 1 / s.
__device__ __forceinline__ float amax_frame_scale(const unsigned* const (&amax)[2], int nseg,
                                                  int frame, float& sinv) {
  unsigned mb = 0;
  for (int sg = 0; sg < nseg; ++sg)
    if (amax[sg]) {
      const unsigned* p = amax[sg] + (size_t)frame * SFA_AMAX_WORDS;
#pragma unroll
      for (int j = 0; j < SFA_AMAX_SHARDS; ++j) mb = max(mb, p[j * SFA_AMAX_STRIDE]);
    }
  if (mb == 0 || mb >= 0x7f800000u) {
    sinv = 1.f;
    return 1.f;
  }
  int e = (int)(mb >> 23) - 127;
  e = e < -100 ? -100 : (e > 100 ? 100 : e);
  sinv = __uint_as_float((unsigned)(127 - 13 + e) << 23);
  return __uint_as_float((unsigned)(127 + 13 - e) << 23);
}

// The same scale from the float bits of a max |x| (a tile's own maximum).
__device__ __forceinline__ float amax_scale_bits(unsigned mb, float& sinv) {
  if (mb == 0 || mb >= 0x7f800000u) {
    sinv = 1.f;
    return 1.f;
  }
  int e = (int)(mb >> 23) - 127;
  e = e < -100 ? -100 : (e > 100 ? 100 : e);
  sinv = __uint_as_float((unsigned)(127 - 13 + e) << 23);
  return __uint_as_float((unsigned)(127 + 13 - e) << 23);
}

// The scales of frames f0 and f1 (both < the batch's frame count) with all their words loaded before
// the first is reduced: one load round trip instead of two (round 5).
__device__ __forceinline__ void amax_frame_scale2(const unsigned* const (&amax)[2], int nseg, int f0, int f1,
                                                  float& s0, float& i0, float& s1, float& i1) {
  if (!amax[0]) {  // (not produced by this launcher: kept exact anyway)
    s0 = amax_frame_scale(amax, nseg, f0, i0);
    s1 = amax_frame_scale(amax, nseg, f1, i1);
    return;
  }
  const bool on1 = nseg > 1 && amax[1];
  const unsigned* p0 = amax[0] + (size_t)f0 * SFA_AMAX_WORDS;
  const unsigned* p1 = amax[0] + (size_t)f1 * SFA_AMAX_WORDS;
  unsigned w[2 * SFA_AMAX_SHARDS];
#pragma unroll
  for (int j = 0; j < SFA_AMAX_SHARDS; ++j) {
    w[j] = p0[j * SFA_AMAX_STRIDE];
    w[SFA_AMAX_SHARDS + j] = p1[j * SFA_AMAX_STRIDE];
  }
  if (on1) {
    const unsigned* q0 = amax[1] + (size_t)f0 * SFA_AMAX_WORDS;
    const unsigned* q1 = amax[1] + (size_t)f1 * SFA_AMAX_WORDS;
#pragma unroll
    for (int j = 0; j < SFA_AMAX_SHARDS; ++j) {
      w[j] = max(w[j], q0[j * SFA_AMAX_STRIDE]);
      w[SFA_AMAX_SHARDS + j] = max(w[SFA_AMAX_SHARDS + j], q1[j * SFA_AMAX_STRIDE]);
    }
  }
#pragma unroll
  for (int h = SFA_AMAX_SHARDS / 2; h >= 1; h >>= 1)
#pragma unroll
    for (int j = 0; j < h; ++j) {
      w[j] = max(w[j], w[j + h]);
      w[SFA_AMAX_SHARDS + j] = max(w[SFA_AMAX_SHARDS + j], w[SFA_AMAX_SHARDS + j + h]);
    }
  const unsigned mb0 = w[0], mb1 = w[SFA_AMAX_SHARDS];
  s0 = amax_scale_bits(mb0, i0);
  s1 = amax_scale_bits(mb1, i1);
}

// Producer side of a conv epilogue (rows m of the output, P = OH * OW rows per frame):
// frames fb0 and fb0 + 1 are reduced over the block, rows of later frames (blocks taller
// than a frame: small maps) are committed one by one.
struct AmaxRows {
  int P, fb0, mb1, mb2;
  float mx0 = 0.f, mx1 = 0.f;
  __device__ AmaxRows(int P_, int m0) : P(P_), fb0(m0 / P_), mb1((m0 / P_ + 1) * P_), mb2(mb1 + P_) {}
  __device__ __forceinline__ void add(unsigned* amax, int m, float val) {
    const float v = fabsf(val);
    if (m < mb1)
      mx0 = fmaxf(mx0, v);
    else if (m < mb2)
      mx1 = fmaxf(mx1, v);
    else if (v > 0.f)
      amax_atomic(amax, m / P, v);
  }
};

// n / d by make_fast_div's multiply-high (conv_args.h)
__device__ __forceinline__ int fast_div(int n, FastDiv f) {
  return (int)((__umulhi((unsigned)n, f.m) + (unsigned)n) >> f.s);
}

// Bilinear x2 (align_corners) sample of a half-resolution NHWC tensor at output pixel
// (b, oh, ow), channel n — F.interpolate(scale_factor=2, mode='bilinear', align_corners=True)
// as upsample2x_bilinear_kernel evaluates it.
__device__ __forceinline__ float res_up_sample(const ConvArgs& a, int m, int n) {
  const int ow = m % a.OW, t = m / a.OW;
  const int oh = t % a.OH, b = t / a.OH;
  const int H = a.OH >> 1, W = a.OW >> 1;
  const float fy = a.res_sh * (float)oh, fx = a.res_sw * (float)ow;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
  const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const float* r = a.res_up + (size_t)b * H * W * a.N + n;
  const float a00 = r[(y0 * W + x0) * a.N], a01 = r[(y0 * W + x1) * a.N];
  const float a10 = r[(y1 * W + x0) * a.N], a11 = r[(y1 * W + x1) * a.N];
  return fmaf(ly0, fmaf(lx0, a00, lx1 * a01), ly1 * fmaf(lx0, a10, lx1 * a11));  // as r3t_epilogue_std
}

int launch_deconv(const DeconvArgs& a, int B, hipStream_t stream);

int launch_conv(const ConvArgs& a, int epilogue, int math, hipStream_t stream);
// fp16x3 stem 7x7/s2 + BN + ReLU + max-pool 3x3/s2 in one kernel over 16 x 16 patches + a merge
// pass (stem_patch_kernel.h); SFA_E_UNSUPPORTED if the stem's shape does not tile 16 x 16.
int launch_stem_patch(const ConvArgs& a, hipStream_t stream);

// One KFPN level's head parameters inside a model handle's packed weights (model.hip), for
// sfa_model_heads_grad (heads_grad.hip): the 3x3 convs of all heads as one [64 heads][9 Cin] float32 matrix
// (K order kh, kw, c), their biases, that matrix's fp16x3 terms and row scales, the 1x1 convs [head][4][64] and their biases [head][4].
// SFA_E_INVALID for a level outside the model's, SFA_E_UNSUPPORTED for a SFA_BACKBONE_DECONV model.
struct HeadsLevel {
  const float *w3, *b3, *w1, *b1;
  const uint16_t* wh;  // the 3x3 matrix's fp16x3 terms [2][64 heads][9 Cin]
  const float* winv;   // [64 heads]
  int Cin, num_heads;
  int ch[SFA_MAX_HEADS];
};
int model_heads_level(const sfa_model* m, int level, HeadsLevel* out);

// conv_up_level{f + 1} inside a model handle's packed weights, for sfa_model_neck_forward / sfa_model_neck_grad
// (neck.hip): the float32 (N, K) matrix in torch's (out, in) order and its bias.
// SFA_E_INVALID for f outside 0..2, SFA_E_UNSUPPORTED for a SFA_BACKBONE_DECONV model.
struct FpnLevel {
  const float *w, *b;
  int N, K;
};
int model_fpn_level(const sfa_model* m, int f, FpnLevel* out);

// BasicBlock layer{layer}.{block} (layer 1..4, block 0, 1) inside a model handle's packed weights, for
// sfa_model_block_forward / sfa_model_block_grad (block.hip): per convolution c = 0 (conv1 + bn1), 1 (conv2 + bn2,
// with downsample.0 + downsample.1 as the columns from kds on when the block has one) the BN-folded float32 rows
// [o][(kh * 3 + kw) C + c] of K[c] words, the folded shift, and the bf16x6 / fp16x3 forms launch_conv reads.
// SFA_E_INVALID for a layer or block out of range, SFA_E_UNSUPPORTED for a SFA_BACKBONE_DECONV model.
struct BlockLevel {
  const float *w[2], *b[2], *winv[2];
  const uint16_t *wx[2], *wh[2];
  int K[2];
  int cin, cout, stride, downsample, kds;
};
int model_block_level(const sfa_model* m, int layer, int block, BlockLevel* out);

// The stem (conv1 + bn1, 7x7 / stride 2 / pad 3, input channels padded 3 -> 4) inside a model handle's packed weights,
// for sfa_model_stem_forward / sfa_model_stem_grad (stem_grad.hip): the BN-folded float32 rows [o][(kh * 7 + kw) 4 + c]
// of K words (zero padded past 196), the folded shift, and the bf16x6 / fp16x3 forms launch_conv reads.  Both backbone
// families share it.
struct StemLevel {
  const float *w, *b, *winv;
  const uint16_t *wx, *wh;
  int K;
};
int model_stem_level(const sfa_model* m, StemLevel* out);

// max |x| of each of B frames of n4 float4s into the frames' records (heads_amax_kernel, heads_grad.hip): what an
// fp16x3 convolution on a caller's map reads as amax_in, measured without atomics or a zeroed record.
int launch_frame_amax(const float* x, unsigned* amax, int B, int n4, hipStream_t st);

}  // namespace sfa
