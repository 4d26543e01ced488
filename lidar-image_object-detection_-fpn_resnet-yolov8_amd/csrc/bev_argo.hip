// Argoverse BEV voxelisation: makeBVFeature on the GPU, for a ragged batch of sweeps.
//
// Reference: argoverse_test2.py:198-257 makeBVFeature(points, discretization, boundary)
//            (argoverse_test.py:199-254 is the same function).
//
// Per kept point (closed box test on all six sides, f32 like numpy on float32 points):
//   row = clip(trunc((maxX - x) / d), 0, H - 1), col = clip(trunc((y - minY) / d), 0, W - 1)
//   h[cell] = max(h[cell], z - minZ), i[cell] = max(i[cell], intensity)  (both start at 0:
//   Python's max(a, b) keeps a unless b > a, so a negative or NaN intensity never wins), n[cell] += 1
// and per frame the channels (density, height, intensity) =
//   (min(n / 10, 1), h / f32(maxZ - minZ), i / max over the frame's cells of i  [if that is > 0]).
// Both maxima are over values >= +0, so an unsigned max of the f32 bits is the float max, and with
// the count it is order-free: every path below gives the same bits as the Python loop.
//
// Record path (default): as the KITTI voxeliser's blocked-bin form (bev.hip).
//   bin    block j of a frame takes its points [1024 j, 1024 j + 1024) and writes the kept ones as
//          records {z bits, intensity bits} + {cell within the strip} into ITS OWN 1024-record
//          region, grouped by strip (SR map rows, SR W <= 4096 cells), with one table word per
//          strip: (first record) | (count << 16).  The block's largest intensity goes to the
//          frame's word with one no-return atomicMax.
//   strip  one block per (frame, strip): scans its table column, reduces the runs in LDS (two
//          ds_max_u32 and one ds_add_u32 per record), divides by the frame's maximum and stores
//          every cell of the strip in the requested layout.
//   tail   the frames' maximum words are zeroed again.
// Atomic path (the batch's records do not fit the scratch, or SFA_ARGO_BEV_FORCE_ATOMIC): two
// atomicMax + one atomicAdd per kept point on a 12-B-per-cell scratch, then one thread per cell,
// which also re-zeroes the cell.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "aux_kernels.h"
#include "bev_plan.h"
#include "dispatch.h"

namespace sfa {

// the limits the scratch plan uses (strip cells, rows and count, points and regions): bev_plan.h
constexpr int kArgoBlkThreads = 256;
constexpr int kArgoPPT = kArgoBlkPts / kArgoBlkThreads;  // 4
constexpr int kArgoStripThreads = 512;
static_assert(kArgoMaxStrips == kArgoPPT * kArgoBlkThreads, "the bin pass scans 4 strips per thread");

struct ArgoArgs {
  int64_t start[SFA_BEV_MAX_BATCH + 1];
  float minX, maxX, minY, maxY, minZ, maxZ;
  float disc;     // f32(discretization)
  float z_range;  // f32(maxZ - minZ), the difference taken in double
  int H, W, stride;
  int strip_rows, strips;  // SR, ceil(H / SR)
};

struct ArgoRecScratch {
  uint2* zi;             // [total blocks][1024]: z - minZ bits, intensity bits
  unsigned short* cell;  // [total blocks][1024]: cell within the strip
  unsigned* tab;         // [strips][total blocks]: first | count << 16
  int nblk_total;
  int blk0[SFA_BEV_MAX_BATCH + 1];
};

// (N, 3) points get intensity 0.5 (:201-203); wider rows use columns 0..3 (:204-205)
template <bool VEC4>
__device__ __forceinline__ float4 argo_load_point(const float* __restrict__ pts, int stride, int64_t i) {
  if (VEC4) return reinterpret_cast<const float4*>(pts)[i];
  const float* p = pts + i * stride;
  return make_float4(p[0], p[1], p[2], stride >= 4 ? p[3] : 0.5f);
}

// The cell and the two values of a point (false: outside the closed box, :210-212; NaN fails).
__device__ __forceinline__ bool argo_point_cell(const float4 p, const ArgoArgs& a, int& row, int& col,
                                                unsigned& zbits, unsigned& ibits) {
  if (!(p.x >= a.minX && p.x <= a.maxX && p.y >= a.minY && p.y <= a.maxY && p.z >= a.minZ && p.z <= a.maxZ))
    return false;
  row = (int)__fdiv_rn(__fsub_rn(a.maxX, p.x), a.disc);  // :230, astype(int32) truncates
  col = (int)__fdiv_rn(__fsub_rn(p.y, a.minY), a.disc);  // :231
  row = min(max(row, 0), a.H - 1);
  col = min(max(col, 0), a.W - 1);
  const float zr = __fsub_rn(p.z, a.minZ);           // :240, >= 0 after the box test
  zbits = zr > 0.f ? __float_as_uint(zr) : 0u;       // -0 -> +0
  ibits = p.w > 0.f ? __float_as_uint(p.w) : 0u;     // :243 max(0, i): negative, -0 and NaN never win
  return true;
}

// The block's largest intensity bits -> the frame's word (one no-return atomic per block).
// Every thread of the block calls it; *smax was zeroed before an earlier __syncthreads().
__device__ __forceinline__ void argo_block_max(unsigned m, unsigned* smax, unsigned* frame_word) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, d, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(smax, m);
  __syncthreads();
  if (threadIdx.x == 0 && *smax) atomicMax(frame_word, *smax);
}

// One output cell (:247-256): channels (density, height, intensity).
template <int LAYOUT>
__device__ __forceinline__ void argo_store_cell(const ArgoArgs& a, int b, int cell, unsigned cnt, unsigned zbits,
                                                unsigned ibits, float frame_max, void* __restrict__ out) {
  const float dens = fminf(__fdiv_rn((float)cnt, 10.0f), 1.0f);  // :247
  const float h = __uint_as_float(zbits), iv = __uint_as_float(ibits);
  // :250-251 divides when any h > 0; a cell with h == 0 stays 0 either way
  const float height = h > 0.f ? __fdiv_rn(h, a.z_range) : 0.f;
  const float inten = frame_max > 0.f ? __fdiv_rn(iv, frame_max) : iv;  // :252-253 (iv == 0 when the max is 0)
  const size_t cells = (size_t)a.H * a.W;
  if (LAYOUT == SFA_BEV_NHWC4_F32) {
    reinterpret_cast<float4*>(out)[(size_t)b * cells + cell] = make_float4(dens, height, inten, 0.f);
  } else {
    float* o = reinterpret_cast<float*>(out) + (size_t)b * 3 * cells + cell;
    o[0] = dens;
    o[cells] = height;
    o[2 * cells] = inten;
  }
}

// ------------------------------------------------------------- atomic path --
template <bool VEC4>
__global__ void __launch_bounds__(256) argo_scatter_kernel(const float* __restrict__ pts, ArgoArgs a,
                                                           unsigned* __restrict__ cells3,
                                                           unsigned* __restrict__ fmax) {
  __shared__ unsigned smax;
  const int b = blockIdx.y;
  const int64_t s = a.start[b];
  const int64_t n = a.start[b + 1] - s;
  if ((int64_t)blockIdx.x * blockDim.x >= n) return;  // the grid fits the largest frame
  if (threadIdx.x == 0) smax = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned m = 0u;
  if (i < n) {
    int row, col;
    unsigned zb, ib;
    if (argo_point_cell(argo_load_point<VEC4>(pts, a.stride, s + i), a, row, col, zb, ib)) {
      unsigned* c = cells3 + ((size_t)b * a.H * a.W + (size_t)row * a.W + col) * 3;
      if (zb) atomicMax(c + 0, zb);
      if (ib) atomicMax(c + 1, ib);
      atomicAdd(c + 2, 1u);
      m = ib;
    }
  }
  argo_block_max(m, &smax, fmax + b);
}

template <int LAYOUT>
__global__ void __launch_bounds__(256) argo_gather_kernel(ArgoArgs a, unsigned* __restrict__ cells3,
                                                          const unsigned* __restrict__ fmax,
                                                          void* __restrict__ out) {
  const int b = blockIdx.y;
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= a.H * a.W) return;
  unsigned* c = cells3 + ((size_t)b * a.H * a.W + cell) * 3;
  const unsigned cnt = c[2];
  unsigned zb = 0u, ib = 0u;
  if (cnt) {
    zb = c[0];
    ib = c[1];
    c[0] = 0u;  // leave the scratch zeroed for the next call
    c[1] = 0u;
    c[2] = 0u;
  }
  argo_store_cell<LAYOUT>(a, b, cell, cnt, zb, ib, __uint_as_float(fmax[b]), out);
}

// ------------------------------------------------------------- record path --
template <bool VEC4>
__global__ void __launch_bounds__(kArgoBlkThreads) argo_bin_kernel(const float* __restrict__ pts, ArgoArgs a,
                                                                   ArgoRecScratch rs,
                                                                   unsigned* __restrict__ fmax) {
  __shared__ unsigned hist[kArgoMaxStrips], first[kArgoMaxStrips];
  __shared__ unsigned wsum[kArgoBlkThreads / 64];
  __shared__ unsigned smax;
  const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  const int NS = a.strips, SR = a.strip_rows;
  const int64_t s = a.start[b];
  const int64_t n = a.start[b + 1] - s;
  if ((int64_t)j * kArgoBlkPts >= n) return;  // past this frame's points (the grid fits the largest)
  for (int t = tid; t < NS; t += kArgoBlkThreads) hist[t] = 0u;
  if (tid == 0) smax = 0u;
  __syncthreads();
  int strip[kArgoPPT];
  unsigned zb[kArgoPPT], ib[kArgoPPT], sc[kArgoPPT], slot[kArgoPPT];
  bool ok[kArgoPPT];
  unsigned m = 0u;
#pragma unroll
  for (int q = 0; q < kArgoPPT; ++q) {
    const int64_t i = (int64_t)j * kArgoBlkPts + q * kArgoBlkThreads + tid;
    int row = 0, col = 0;
    ok[q] = i < n && argo_point_cell(argo_load_point<VEC4>(pts, a.stride, s + i), a, row, col, zb[q], ib[q]);
    strip[q] = ok[q] ? row / SR : 0;
    sc[q] = (unsigned)((row - strip[q] * SR) * a.W + col);
    slot[q] = ok[q] ? atomicAdd(&hist[strip[q]], 1u) : 0u;
    if (ok[q]) m = max(m, ib[q]);
  }
  __syncthreads();
  {  // exclusive scan of the strip counts: thread t owns strips 4 t .. 4 t + 3
    unsigned c[kArgoPPT], sum = 0u;
#pragma unroll
    for (int q = 0; q < kArgoPPT; ++q) {
      c[q] = kArgoPPT * tid + q < NS ? hist[kArgoPPT * tid + q] : 0u;
      sum += c[q];
    }
    unsigned x = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned y = __shfl_up(x, d, 64);
      if ((tid & 63) >= d) x += y;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = x;
    __syncthreads();
    unsigned e = x - sum;
    for (int w = 0; w < (tid >> 6); ++w) e += wsum[w];
#pragma unroll
    for (int q = 0; q < kArgoPPT; ++q) {
      if (kArgoPPT * tid + q < NS) first[kArgoPPT * tid + q] = e;
      e += c[q];
    }
  }
  __syncthreads();
  const size_t region = (size_t)(rs.blk0[b] + j);
  for (int t = tid; t < NS; t += kArgoBlkThreads) rs.tab[(size_t)t * rs.nblk_total + region] = first[t] | (hist[t] << 16);
#pragma unroll
  for (int q = 0; q < kArgoPPT; ++q)
    if (ok[q]) {
      const size_t r = region * kArgoBlkPts + first[strip[q]] + slot[q];
      rs.zi[r] = make_uint2(zb[q], ib[q]);
      rs.cell[r] = (unsigned short)sc[q];
    }
  argo_block_max(m, &smax, fmax + b);
}

template <int LAYOUT>
__global__ void __launch_bounds__(kArgoStripThreads) argo_strip_kernel(ArgoArgs a, ArgoRecScratch rs,
                                                                       const unsigned* __restrict__ fmax,
                                                                       void* __restrict__ out) {
  constexpr int NT = kArgoStripThreads, MAXR = kArgoMaxRegions;
  constexpr int RPT = MAXR / NT;  // table words per thread (at most)
  __shared__ unsigned sz[kArgoStripCells], si[kArgoStripCells], sn[kArgoStripCells];
  __shared__ unsigned pre[MAXR + 1];  // this strip's records before region r
  __shared__ unsigned short first[MAXR];
  __shared__ unsigned wsum[NT / 64];
  const int strip = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int SC = a.strip_rows * a.W;  // <= kArgoStripCells
  for (int c = tid; c < SC; c += NT) {
    sz[c] = 0u;
    si[c] = 0u;
    sn[c] = 0u;
  }
  const int nblk = rs.blk0[b + 1] - rs.blk0[b];  // <= MAXR (checked at launch)
  const size_t reg0 = (size_t)rs.blk0[b];
  const unsigned* col = rs.tab + (size_t)strip * rs.nblk_total + reg0;
  // exclusive scan of the regions' counts of this strip: thread t owns regions [t*per, t*per+per)
  const int per = (nblk + NT - 1) / NT;
  unsigned wv[RPT];
  unsigned loc = 0;
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int r = tid * per + q;
    wv[q] = q < per && r < nblk ? col[r] : 0u;
    loc += wv[q] >> 16;
  }
  unsigned x = loc;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned y = __shfl_up(x, d, 64);
    if ((tid & 63) >= d) x += y;
  }
  if ((tid & 63) == 63) wsum[tid >> 6] = x;
  __syncthreads();  // also: sz / si / sn written
  unsigned run = x - loc;
  for (int w = 0; w < (tid >> 6); ++w) run += wsum[w];
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int r = tid * per + q;
    if (q < per && r < nblk) {
      pre[r] = run;
      first[r] = (unsigned short)(wv[q] & 0xffffu);
      run += wv[q] >> 16;
    }
  }
  if (tid == NT - 1) {  // the total: every thread's count
    unsigned t = 0;
    for (int w = 0; w < NT / 64; ++w) t += wsum[w];
    pre[nblk] = t;
  }
  __syncthreads();
  const unsigned total = pre[nblk];
  // every record of the strip, 4 per thread per round: region by binary search over pre, the
  // loads in flight together, then the LDS maxima and the count
  for (unsigned base = 0; base < total; base += 4 * NT) {
    uint2 e[4];
    unsigned c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned idx = base + u * NT + tid;
      int lo = 0, hi = nblk - 1;  // last region with pre[r] <= idx
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= idx) lo = mid; else hi = mid - 1;
      }
      e[u] = make_uint2(0u, 0u);
      c[u] = 0u;
      if (idx < total) {
        const size_t r = (reg0 + lo) * kArgoBlkPts + first[lo] + (idx - pre[lo]);
        e[u] = rs.zi[r];
        c[u] = rs.cell[r];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + u * NT + tid < total) {
        if (e[u].x) atomicMax(&sz[c[u]], e[u].x);
        if (e[u].y) atomicMax(&si[c[u]], e[u].y);
        atomicAdd(&sn[c[u]], 1u);
      }
  }
  __syncthreads();
  const float frame_max = __uint_as_float(fmax[b]);
  const int cell0 = strip * SC, ncell = a.H * a.W;  // the last strip may be short
  for (int c = tid; c < SC && cell0 + c < ncell; c += NT)
    argo_store_cell<LAYOUT>(a, b, cell0 + c, sn[c], sz[c], si[c], frame_max, out);
}

// H = int((maxX - minX) / d), W = int((maxY - minY) / d) in double, as Python evaluates :224-225
static int argo_shape(const double* bnd, double d, int* H, int* W) {
  SFA_CHECK_ARG(bnd && H && W, "argo bev: null argument");
  for (int k = 0; k < 6; ++k) SFA_CHECK_ARG(std::isfinite(bnd[k]), "argo bev: boundary[%d] is not finite", k);
  SFA_CHECK_ARG(std::isfinite(d) && d > 0.0, "argo bev: discretization %g is not positive", d);
  SFA_CHECK_ARG(bnd[1] > bnd[0] && bnd[3] > bnd[2] && bnd[5] >= bnd[4],
                "argo bev: inverted boundary (need minX < maxX, minY < maxY, minZ <= maxZ)");
  const double h = (bnd[1] - bnd[0]) / d, w = (bnd[3] - bnd[2]) / d;
  if (!(h >= 1.0 && h < kArgoMaxDim + 1.0 && w >= 1.0 && w < kArgoMaxDim + 1.0)) {
    set_error("argo bev: map of %g x %g cells outside [1, %d] x [1, %d]", h, w, kArgoMaxDim, kArgoMaxDim);
    return SFA_E_UNSUPPORTED;
  }
  *H = (int)h;
  *W = (int)w;
  return SFA_OK;
}

}  // namespace sfa

using namespace sfa;

extern "C" int sfa_argo_bev_shape(const double* boundary, double discretization, int* H, int* W) {
  return argo_shape(boundary, discretization, H, W);
}

// The scratch's halves and the choice of the path: argo_plan (bev_plan.h).
extern "C" size_t sfa_argo_bev_scratch_size(int batch, int H, int W) { return argo_scratch_size(batch, H, W); }

namespace {

// What the launches of both paths share.
struct ArgoCall {
  const float* pts;
  ArgoArgs a;
  int batch, layout;
  int64_t max_n;  // points of the largest frame
  bool vec4;      // one aligned float4 per point
  void* out;
  char* scratch;
  hipStream_t st;
  template <typename T>
  T* at(const Region& r) const { return reinterpret_cast<T*>(scratch + r.off); }
};

int argo_records(const ArgoCall& c, const ArgoPlan& p) {
  ArgoRecScratch rs;
  rs.zi = c.at<uint2>(p.zi);
  rs.cell = c.at<unsigned short>(p.cell);
  rs.tab = c.at<unsigned>(p.tab);
  rs.nblk_total = p.nblk_total;
  std::copy(p.blk0, p.blk0 + c.batch + 1, rs.blk0);
  unsigned* fmax = c.at<unsigned>(p.fmax);
  if (c.max_n > 0) {
    const dim3 g1((unsigned)((c.max_n + kArgoBlkPts - 1) / kArgoBlkPts), c.batch);
    if (int rc = with_bool(c.vec4, [&](auto VEC4) {
          return launch({g1, dim3(kArgoBlkThreads), c.st}, argo_bin_kernel<VEC4.value>, c.pts, c.a, rs, fmax);
        }))
      return rc;
  }
  const dim3 g2(c.a.strips, c.batch);
  return with_f32_layout(c.layout, [&](auto L) {
    return launch({g2, dim3(kArgoStripThreads), c.st}, argo_strip_kernel<L.value>, c.a, rs, fmax, c.out);
  });
}

int argo_atomic(const ArgoCall& c, const ArgoPlan& p) {
  unsigned* fmax = c.at<unsigned>(p.fmax);
  unsigned* cells3 = c.at<unsigned>(p.cells3);
  if (c.max_n > 0) {
    const int64_t nb = (c.max_n + 255) / 256;
    if (nb > INT32_MAX) {
      set_error("argo bev: a frame of %lld points is beyond the launch grid", (long long)c.max_n);
      return SFA_E_UNSUPPORTED;
    }
    const dim3 g1((unsigned)nb, c.batch);
    if (int rc = with_bool(c.vec4, [&](auto VEC4) {
          return launch({g1, dim3(256), c.st}, argo_scatter_kernel<VEC4.value>, c.pts, c.a, cells3, fmax);
        }))
      return rc;
  }
  const dim3 g2((unsigned)ceil_div(c.a.H * c.a.W, 256), c.batch);
  return with_f32_layout(c.layout, [&](auto L) {
    return launch({g2, dim3(256), c.st}, argo_gather_kernel<L.value>, c.a, cells3, fmax, c.out);
  });
}

// The frames' starts and the largest frame.
int argo_fill_frames(const float* points, const int64_t* frame_offsets, int batch, ArgoArgs* a, int64_t* max_n) {
  SFA_CHECK_ARG(frame_offsets[0] >= 0, "argo bev: negative frame offset");
  *max_n = 0;
  for (int b = 0; b <= batch; ++b) {
    a->start[b] = frame_offsets[b];
    if (b > 0) {
      const int64_t n = frame_offsets[b] - frame_offsets[b - 1];
      SFA_CHECK_ARG(n >= 0, "argo bev: frame_offsets not monotone at %d", b);
      if (n >= (int64_t)0xffffffff) {  // the per-cell count is 32 bits
        set_error("argo bev: frame %d has %lld points (< 2^32 - 1 supported)", b - 1, (long long)n);
        return SFA_E_UNSUPPORTED;
      }
      *max_n = std::max(*max_n, n);
    }
  }
  SFA_CHECK_ARG(*max_n == 0 || points, "argo bev: null points");
  return SFA_OK;
}

}  // namespace

extern "C" int sfa_argo_bev_voxelize(const float* points, int point_stride, const int64_t* frame_offsets, int batch,
                                     const double* boundary, double discretization, int out_layout, void* out,
                                     void* scratch, size_t scratch_bytes, void* stream) {
  SFA_CHECK_ARG(batch >= 1 && batch <= SFA_BEV_MAX_BATCH, "argo bev: batch %d out of [1, %d]", batch,
                SFA_BEV_MAX_BATCH);
  SFA_CHECK_ARG(frame_offsets && boundary && out && scratch, "argo bev: null argument");
  SFA_CHECK_ARG(point_stride >= 3, "argo bev: point_stride %d (floats per point: 3 or >= 4)", point_stride);
  const bool force_atomic = (out_layout & SFA_ARGO_BEV_FORCE_ATOMIC) != 0;
  ArgoCall c;
  c.layout = out_layout & ~SFA_ARGO_BEV_FORCE_ATOMIC;
  SFA_CHECK_ARG(c.layout == SFA_BEV_NCHW3_F32 || c.layout == SFA_BEV_NHWC4_F32,
                "argo bev: out_layout %d (SFA_BEV_NCHW3_F32 or SFA_BEV_NHWC4_F32)", out_layout);
  ArgoArgs& a = c.a;
  if (int rc = argo_shape(boundary, discretization, &a.H, &a.W)) return rc;
  if (int rc = argo_fill_frames(points, frame_offsets, batch, &a, &c.max_n)) return rc;
  SFA_CHECK_ARG(reinterpret_cast<uintptr_t>(scratch) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(points) % 4 == 0,
                "argo bev: misaligned buffer (scratch / out: 16 B, points: 4 B)");
  const size_t need = argo_scratch_size(batch, a.H, a.W);
  if (scratch_bytes < need) {
    set_error("argo bev: scratch of %zu bytes, %d frames of %d x %d need %zu (sfa_argo_bev_scratch_size)",
              scratch_bytes, batch, a.H, a.W, need);
    return SFA_E_WORKSPACE;
  }
  const ArgoPlan p = argo_plan(scratch_bytes, batch, frame_offsets, a.H, a.W, force_atomic);
  // Python floats -> f32 as numpy does for ops with a float32 array
  a.minX = (float)boundary[0];
  a.maxX = (float)boundary[1];
  a.minY = (float)boundary[2];
  a.maxY = (float)boundary[3];
  a.minZ = (float)boundary[4];
  a.maxZ = (float)boundary[5];
  a.disc = (float)discretization;
  a.z_range = (float)(boundary[5] - boundary[4]);
  a.stride = point_stride;
  a.strip_rows = p.strip_rows;
  a.strips = p.strips;
  c.pts = points;
  c.batch = batch;
  c.vec4 = point_stride == 4 && reinterpret_cast<uintptr_t>(points) % 16 == 0;
  c.out = out;
  c.scratch = reinterpret_cast<char*>(scratch);
  c.st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = p.records ? argo_records(c, p) : argo_atomic(c, p)) return rc;
  // the frames' maxima back to zero (only a pass over points can have raised them)
  if (c.max_n > 0) return launch_zero_words(c.at<unsigned>(p.fmax), (size_t)batch * sizeof(unsigned), c.st);
  return SFA_OK;
}
