// Transposed convolution ConvTranspose2d(C, N, k=4, s=2, p=1) + folded BatchNorm + ReLU, fp16x3
// arithmetic, for gfx950 (the three upsampling layers of the plain resnet_18 detector,
// models/resnet.py:192-217).
//
// Phase decomposition: with oy = 2 iy - 1 + ky, the outputs of one parity (py, px) = (oy & 1, ox & 1)
// are a dense 2 x 2 convolution of the input — no zero-stuffed MACs:
//   oy = 2q     <- (ky 1, iy q), (ky 3, iy q - 1)        oy = 2q + 1 <- (ky 2, iy q), (ky 0, iy q + 1)
// i.e. tap dy in {0, 1} reads iy = q - 1 + py + dy with ky = 3 - py - 2 dy (columns alike); an iy / ix
// outside the input contributes zero.  Each phase is an implicit GEMM C[M][N] = A[M][K] W[N][K]^T with
// M = B h w (one row per INPUT pixel (b, q, r)), K = 4 C ordered (dy, dx, c), written to
// y[b][2q + py][2r + px][:].  One launch covers the four phases: block -> (phase, M-tile, N-tile), so
// the smallest layer (19 x 19 at 608 x 608, 16 frames: 4 x 46 x 2 = 368 tiles) still fills the chip.
//
// The GEMM core is conv_h3_kernel's 16x16x32 form (conv_h3_kernel.h): A (f32) gathered with LDS-DMA
// into a two-stage ring and split into two fp16 terms (x s = hi + lo, s the frame's power-of-two scale
// from the producer's amax words) when a wave reads its fragment; W pre-split on the host per phase
// and packed row (split_terms_h3); products hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16 with f32
// accumulation; the same LDS images and swizzles.  The epilogue scales back (1 / s of the row's frame,
// winv[n]), adds the bias (the BN shift), applies ReLU, stores the phase's pixels and records the
// output's per-frame max |y| for the next layer / the heads.  A row's arithmetic depends only on its
// own frame's scale and the fixed K order, so frames are batch-invariant.
#pragma once

#include "conv_h3_kernel.h"

namespace sfa {

template <int BM, int BN, int WM, int OCC>
__global__ void __launch_bounds__((BM / WM) * 64, OCC) deconv_h3_kernel(const DeconvArgs a) {
  constexpr int BK = 32, NSTAGE = 2;
  constexpr int NW = BM / WM;
  constexpr int TM = WM / 16, TN = BN / 16;
  constexpr int AROW = BK * 4, BROW = BK * 2;  // bytes per LDS row
  constexpr int A_BYTES = BM * AROW, TERM_B = BN * BROW;
  constexpr int STAGE = A_BYTES + 2 * TERM_B;
  constexpr int A_RPD = 1024 / AROW, B_RPD = 1024 / BROW;  // rows per DMA instruction
  constexpr int ND_A = BM / A_RPD, ND_BT = BN / B_RPD, ND_B = 2 * ND_BT;
  static_assert(ND_A % NW == 0 && ND_B % NW == 0 && NW % 2 == 0 && WM % 16 == 0 && BN % 16 == 0, "tile");
  constexpr int NA = ND_A / NW, NB = ND_B / NW;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NSTAGE * STAGE];

  // LDS images of conv_h3_kernel's 16x16x32 form: 16-B quad / chunk q of row R stored at q ^ swz(R)
  auto swzA = [](int R) { return ((R >> 1) & 7) ^ ((((R & 15) + 4) >> 2) & 2); };
  auto swzB = [](int R) { return ((R >> 2) & 3) ^ ((((R & 15) + 4) >> 3) & 1); };

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_tiles = a.N / BN;
  const int m_tiles = (a.M + BM - 1) / BM;
  int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int ph = lbid / (m_tiles * n_tiles);  // 2 py + px
  lbid -= ph * (m_tiles * n_tiles);
  const int mt = lbid / n_tiles, nt = lbid - mt * n_tiles;
  const int py = ph >> 1, px = ph & 1;
  const int m0 = mt * BM, n0 = nt * BN;
  const int M = a.M, P = a.H * a.W;

  // ---- A DMA slots: groups d = wave + NW * i, rows A_RPD * d + lane / QPR ----
  constexpr int QPR = AROW / 16;
  const int arow_in = lane / QPR;
  const int kq = (lane % QPR) ^ swzA(A_RPD * wave + arow_in);
  int r_pix[NA], r_ihw[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int m = m0 + A_RPD * (wave + NW * i) + arow_in;
    const bool ok = m < M;
    const int mm = ok ? m : 0;
    const int t = fast_div(mm, a.fd_w);
    const int r = mm - t * a.W;
    const int b = fast_div(t, a.fd_h);
    const int q = t - b * a.H;
    const int ih = ok ? q - 1 + py : -16384;  // tap dy reads row ih + dy
    const int iw = r - 1 + px;
    r_pix[i] = (b * a.H + ih) * a.W + iw;
    r_ihw[i] = (ih << 16) | (iw & 0xffff);
  }
  const __amdgpu_buffer_rsrc_t rsx =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), (short)0, (int)a.bytes, 0x00020000);

  // ---- W DMA slots: groups e = wave + NW * j (term e / ND_BT, rows (e % ND_BT) * B_RPD + ..) ----
  const unsigned term_bytes = (unsigned)a.N * (unsigned)a.K * 2u;
  const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(a.wh + (size_t)ph * 2 * a.N * a.K), (short)0, (int)(2 * term_bytes), 0x00020000);
  const float* winv = a.winv + ph * a.N;
  constexpr int CPR = BROW / 16;
  int boff[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int e = wave + NW * j;
    const int t = e / ND_BT;
    const int R = (e % ND_BT) * B_RPD + lane / CPR;
    const int lc = (lane % CPR) ^ swzB(R);
    boff[j] = (int)(t * term_bytes) + (int)(((n0 + R) * a.K + 8 * lc) << 1);
  }

  // fp16x3 scale of the frame of this lane's A row in each 16-row MFMA tile
  const unsigned* const am_in[2] = {a.amax_in, nullptr};
  float as[TM], ainv[TM];
  {
    const int f0 = m0 / P, fb = (f0 + 1) * P;
    float sA, iA, sB, iB;
    amax_frame_scale2(am_in, 1, f0, min(f0 + 1, (M - 1) / P), sA, iA, sB, iB);
    if (fb >= M) {
      sB = sA;
      iB = iA;
    }
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      const int m = min(m0 + wave * WM + mi * 16 + (lane & 15), M - 1);
      if (m < fb) {
        as[mi] = sA;
        ainv[mi] = iA;
      } else if (m < fb + P) {
        as[mi] = sB;
        ainv[mi] = iB;
      } else {
        as[mi] = amax_frame_scale(am_in, 1, m / P, ainv[mi]);
      }
    }
  }

  auto load_tile = [&](int kt, unsigned char* S) {
    const int k0 = kt * BK;
    const int kk = k0 + 4 * kq;
    const int tap = kk >> a.logC;  // (dy, dx) = (tap >> 1, tap & 1); 32 | C: one tap per K-tile
    const int c = kk & (a.C - 1);
    const int dy = tap >> 1, dx = tap & 1;
    const int toff = dy * a.W + dx;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int ih = r_ihw[i] >> 16;
      const int iw = (int)(short)(r_ihw[i] & 0xffff);
      const bool ok = ((unsigned)(ih + dy) < (unsigned)a.H) & ((unsigned)(iw + dx) < (unsigned)a.W);
      const unsigned off = ok ? (unsigned)((((r_pix[i] + toff) << a.logC) + c) << 2) : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rsx, (__attribute__((address_space(3))) void*)(S + (wave + NW * i) * 1024), 16, off, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rsw, (__attribute__((address_space(3))) void*)(S + A_BYTES + (wave + NW * j) * 1024), 16,
          (unsigned)(boff[j] + 2 * k0), 0, 0, 0);
  };

  f32x4_t acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[mi][ni][v] = 0.f;

  const int c16 = lane & 15, g = lane >> 4;
  // lane l reads A row l & 15 quads 2 (l >> 4), +1 and W row l & 15 chunk l >> 4; the W fragments
  // two column blocks ahead of their MFMAs
  auto compute = [&](const unsigned char* S) {
    f16x8_t hf[2][TM];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      const int R = wave * WM + mi * 16 + c16;
      const x6_f32x4 q0 = *reinterpret_cast<const x6_f32x4*>(S + R * AROW + (((2 * g) ^ swzA(R)) << 4));
      const x6_f32x4 q1 = *reinterpret_cast<const x6_f32x4*>(S + R * AROW + (((2 * g + 1) ^ swzA(R)) << 4));
      split2h_x8(q0, q1, as[mi], hf[0][mi], hf[1][mi]);
    }
    const unsigned char* SB = S + A_BYTES + c16 * BROW + ((g ^ swzB(c16)) << 4);
    f16x8_t bq[3][2];
    auto read_b = [&](int ni) {
      bq[ni % 3][0] = *reinterpret_cast<const f16x8_t*>(SB + ni * 16 * BROW);
      bq[ni % 3][1] = *reinterpret_cast<const f16x8_t*>(SB + TERM_B + ni * 16 * BROW);
    };
    read_b(0);
    if (TN > 1) read_b(1);
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
      if (ni + 2 < TN) read_b(ni + 2);
      const f16x8_t c0 = bq[ni % 3][0], c1 = bq[ni % 3][1];
#pragma unroll
      for (int mi = 0; mi < TM; ++mi) {
        f32x4_t cc = acc[mi][ni];
        cc = __builtin_amdgcn_mfma_f32_16x16x32_f16(hf[1][mi], c0, cc, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_16x16x32_f16(hf[0][mi], c1, cc, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_16x16x32_f16(hf[0][mi], c0, cc, 0, 0, 0);
        acc[mi][ni] = cc;
      }
    }
  };

  // two-stage ring: tile kt lives in stage kt & 1, tile kt + 1 is in flight while kt is multiplied
  const int nk = a.K / BK;
  load_tile(0, smem);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMAs of tile kt have landed
    __builtin_amdgcn_s_barrier();  // every wave's: stage kt complete; stage kt - 1 no longer read
    load_tile(kt + 1 < nk ? kt + 1 : nk - 1, smem + ((kt + 1) & 1) * STAGE);
    compute(smem + (kt & 1) * STAGE);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- epilogue (accumulator layout: lane l, register v -> row 4 (l >> 4) + v, column l & 15) ----
  float rinv[TM][4];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int v = 0; v < 4; ++v) rinv[mi][v] = __shfl(ainv[mi], 4 * g + v, 64);
  float bng[TN], csg[TN];
#pragma unroll
  for (int ni = 0; ni < TN; ++ni) {
    const int n = n0 + ni * 16 + c16;
    bng[ni] = a.bias[n];
    csg[ni] = winv[n];
  }
  AmaxRows am(P, m0);
  const int OW = 2 * a.W;
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = m0 + wave * WM + mi * 16 + 4 * g + v;
      if (m < M) {
        const int t = fast_div(m, a.fd_w);
        const int r = m - t * a.W;  // t = b H + q: output row 2 t + py of the (B 2H) x 2W pixel grid
        float* yrow = a.y + ((size_t)(2 * t + py) * OW + 2 * r + px) * a.N + n0 + c16;
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const float val = fmaxf(acc[mi][ni][v] * rinv[mi][v] * csg[ni] + bng[ni], 0.f);
          yrow[ni * 16] = val;
          if (a.amax_out) am.add(a.amax_out, m, val);
        }
      }
    }
  }
  if (a.amax_out)
    amax_commit_block<NW>(a.amax_out, am.fb0, am.mx0, am.mx1, reinterpret_cast<float*>(smem));
}

// Host-side checks (the kernel assumes them and never bounds-checks) and the launch: 128 x 128 tiles,
// four waves of 32 rows, two blocks per CU.
inline int launch_deconv_h3_cfg(const DeconvArgs& a, int B, hipStream_t st) {
  constexpr int BM = 128, BN = 128, WM = 32;
  unsigned grid;
  if (int rc = deconv_check(a, B, BM, BN, &grid)) return rc;
  DeconvArgs c = a;
  c.fd_w = make_fast_div((unsigned)a.W);
  c.fd_h = make_fast_div((unsigned)a.H);
  return launch({grid, (BM / WM) * 64, st}, deconv_h3_kernel<BM, BN, WM, 2>, c);
}

}  // namespace sfa
