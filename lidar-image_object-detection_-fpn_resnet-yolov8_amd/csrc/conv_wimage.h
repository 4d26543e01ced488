// Pre-tiled LDS images of a conv's fp16 weight terms: plain C++ (no HIP include), shared by the image
// builder (aux_kernels.hip), the kernels' launch checks and the CPU check (tools/wimage_plan_check.cpp).
//
// The fp16x3 kernels stage W in LDS per K-tile as, per term, BN rows of 64 B (32 fp16 K columns), the
// 16-B quad q of row R stored at quad q ^ swzB(R) (conv_r3_kernel.h / conv_h3_kernel.h, the 16x16x32
// form). From the packed row-major terms [term][N][wstride] a 1-KiB LDS-DMA piece is a gather of
// sixteen 64-B row segments. The image holds the same LDS bytes in the kernel's own order:
//   [column tile nt][K-tile kt, in the kernel's K order][piece e][lane l][16 B]
// so piece e of K-tile kt of column tile nt is the 1,024 contiguous bytes at
// ((nt * ktiles + kt) * pieces + e) * 1024 and lane l takes bytes 16 l .. 16 l + 15 of it.
// Piece e holds term e / (BN / 16), rows n0 + 16 (e % (BN / 16)) + l / 4. The packed weights stay as
// they are (the gradient kernels and the other math modes read them): the image is a second buffer,
// built once per (conv, kernel instance) and rebuilt by whoever changes the packed terms.
#pragma once

#include <cstddef>
#include <cstdint>

// the index arithmetic also runs in the builder kernel
#ifdef __HIPCC__
#define SFA_WIMG_FN __host__ __device__ inline
#else
#define SFA_WIMG_FN inline
#endif

namespace sfa {

// One image: the conv's slice of the packed terms and the kernel instance's tile and K order.
struct WImageGeom {
  int N;        // output channels (rows of each packed term)
  int K;        // K columns the kernel sweeps (multiple of 32): the whole conv, or a K-slice
  int wstride;  // row stride of the packed terms, in columns (>= wk0 + K)
  int wk0;      // first column of the slice (0: the whole conv)
  int BN;       // the kernel's tile width (rows of W per tile)
  int terms;    // 2 (fp16x3)
  // chunk-major K order (r3opt::CHUNK_MAJOR) over the first cmaj_tiles K-tiles, a 3x3 window of C
  // channels: K-tile kt covers tap kt % 9 of the 32-channel chunk kt / 9; the tiles after them
  // (a fused 1x1 downsample segment) and every tile of a tap-major kernel (cmaj_tiles 0): kt * 32
  int cmaj_tiles, C;
  // strip K order (conv_h3s_kernel; 0: the orders above): a whole 3x3 window of C channels, K = 9 C,
  // swept as (kh, 32-channel chunk, kw): K-tile kt is tap kw = kt % 3 of super-step s = kt / 3,
  // kh = s / (C / 32), chunk = s % (C / 32). A split-K slice of the launch sweeps a contiguous run of
  // super-steps, so its K-tiles are contiguous in the one image of the conv.
  int strip;
};

constexpr int WIMG_BK = 32;       // K columns per K-tile
constexpr int WIMG_PIECE = 1024;  // bytes of one LDS-DMA piece (64 lanes x 16 B = 16 rows of 64 B)

// the quad swizzle of LDS row R (conv_r3_kernel.h swzB)
SFA_WIMG_FN int wimage_swz(int R) { return ((R >> 2) & 3) ^ ((((R & 15) + 4) >> 3) & 1); }

SFA_WIMG_FN int wimage_ktiles(const WImageGeom& g) { return g.K / WIMG_BK; }
SFA_WIMG_FN int wimage_pieces(const WImageGeom& g) { return g.terms * g.BN * 64 / WIMG_PIECE; }  // per K-tile
SFA_WIMG_FN size_t wimage_tile_bytes(const WImageGeom& g) { return (size_t)wimage_pieces(g) * WIMG_PIECE; }
SFA_WIMG_FN size_t wimage_bytes(const WImageGeom& g) {
  return (size_t)(g.N / g.BN) * (size_t)wimage_ktiles(g) * wimage_tile_bytes(g);
}

// first weight column (inside the slice) of K-tile kt, in the kernel's order (conv_r3_kernel.h kcol)
SFA_WIMG_FN int wimage_kcol(const WImageGeom& g, int kt) {
  if (g.strip) {  // conv_h3s_kernel.h wk0
    const int nchunk = g.C / WIMG_BK, s = kt / 3, kw = kt - 3 * s;
    const int kh = s / nchunk, chunk = s - kh * nchunk;
    return (kh * 3 + kw) * g.C + chunk * WIMG_BK;
  }
  if (kt < g.cmaj_tiles) {
    const int chunk = kt / 9;
    return (kt - 9 * chunk) * g.C + chunk * WIMG_BK;
  }
  return kt * WIMG_BK;
}

// The 16 bytes of (column tile nt, K-tile kt, piece e, lane l): 8 consecutive fp16 of the packed
// terms, starting at element index (term * N + n) * wstride + k of the terms array. Returns that
// index and the parts.
SFA_WIMG_FN size_t wimage_source(const WImageGeom& g, int nt, int kt, int e, int lane, int* term, int* n, int* k) {
  const int nd_bt = g.BN / 16;  // pieces per term
  const int t = e / nd_bt;
  const int R = 16 * (e % nd_bt) + lane / 4;  // LDS row inside the term
  const int q = (lane % 4) ^ wimage_swz(R);   // the source quad stored at LDS quad lane % 4
  const int nn = nt * g.BN + R;
  const int kk = g.wk0 + wimage_kcol(g, kt) + 8 * q;
  if (term) *term = t;
  if (n) *n = nn;
  if (k) *k = kk;
  return ((size_t)t * g.N + nn) * g.wstride + kk;
}

// byte offset of (nt, kt, e, lane) in the image
SFA_WIMG_FN size_t wimage_offset(const WImageGeom& g, int nt, int kt, int e, int lane) {
  return (((size_t)nt * wimage_ktiles(g) + kt) * wimage_pieces(g) + e) * WIMG_PIECE + (size_t)lane * 16;
}

// What the builder and the kernels rely on; null if the geometry is fine, else what is wrong.
inline const char* wimage_check(const WImageGeom& g) {
  if (g.terms != 2) return "wimage: fp16x3 (two terms) only";
  if (g.N <= 0 || g.BN <= 0 || g.BN % 16 != 0 || g.N % g.BN != 0) return "wimage: N is not a multiple of the tile width";
  if (g.K <= 0 || g.K % WIMG_BK != 0) return "wimage: K is not a multiple of 32";
  // 16-B aligned source quads
  if (g.wk0 < 0 || g.wk0 % 8 != 0 || g.wstride % 8 != 0) return "wimage: slice not 16-B aligned";
  if ((long long)g.wk0 + g.K > g.wstride) return "wimage: slice outside the packed rows";
  if (g.cmaj_tiles < 0 || g.cmaj_tiles > wimage_ktiles(g)) return "wimage: chunk-major tiles outside K";
  if (g.cmaj_tiles > 0 && (g.C < WIMG_BK || g.C % WIMG_BK != 0 || g.cmaj_tiles != 9 * (g.C / WIMG_BK)))
    return "wimage: chunk-major order needs a 3x3 window of C % 32 == 0 channels";
  if (g.strip && (g.cmaj_tiles != 0 || g.C < WIMG_BK || g.C % WIMG_BK != 0 || g.K != 9 * g.C))
    return "wimage: strip order needs a whole 3x3 window of C % 32 == 0 channels";
  // the kernels address both buffers with 32-bit byte offsets
  if (wimage_bytes(g) >= (1ull << 31) || 2ull * g.terms * g.N * g.wstride >= (1ull << 31))
    return "wimage: image or terms above 2 GiB";
  return nullptr;
}

// The images of one model in one device buffer: 256-B aligned, disjoint, in the order given.
// MAX: the plan's cap. The heads' plan (WImagePlan) and the body convs' (WBodyImagePlan, a second buffer).
template <int MAX>
struct WImagePlanT {
  int count;
  size_t off[MAX], bytes[MAX];
  size_t total;
};
constexpr int WIMG_MAX = 8;
using WImagePlan = WImagePlanT<WIMG_MAX>;
constexpr int WIMG_BODY_MAX = 16;  // the residual layers have 16 convs
using WBodyImagePlan = WImagePlanT<WIMG_BODY_MAX>;

template <int MAX>
inline const char* wimage_plan(const WImageGeom* g, int count, WImagePlanT<MAX>* p) {
  if (count < 0 || count > MAX) return "wimage: too many images";
  p->count = count;
  size_t cur = 0;
  for (int i = 0; i < count; ++i) {
    if (const char* err = wimage_check(g[i])) return err;
    p->off[i] = cur;
    p->bytes[i] = wimage_bytes(g[i]);
    cur = (cur + p->bytes[i] + 255) / 256 * 256;
  }
  p->total = cur;
  return nullptr;
}

}  // namespace sfa
