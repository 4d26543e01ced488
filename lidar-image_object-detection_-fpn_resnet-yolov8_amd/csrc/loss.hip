// Validation tier on device: the training targets of a batch of label lists
// (data_process/kitti_dataset.py:157-244 build_targets with compute_radius, gaussian2D and
// gen_hm_radius, kitti_data_utils.py:176-225) and the loss of the five head maps against them
// (losses/losses.py:44-163 Compute_Loss), and the gradient of that loss at the five head maps
// (sfa_compute_loss_grad, at the end of the file).  Nothing is differentiated past the head maps.
//
// build_targets is a GATHER.  The reference draws the labels one after the other and an ignore
// label ASSIGNS 0.9999 at its centre, so the map depends on the label order: a later ignore label
// lowers a 1.0, a later gaussian raises a 0.9999 again.  Here every thread owns heat-map cells and
// walks the frame's labels in label order from LDS, applying max or the assignment as the
// reference would: exact for any order, no atomics, every output byte written by the call.
//
// compute_loss: one streaming pass over the B*C*H*W heat-map cells (fixed 4096-cell chunks, one
// per block, partial sums in float64 to the workspace), one pass over the B*M slot rows (256 rows
// per block), one single-block fold in a fixed order.  The partition depends on the shape alone,
// so two runs, eager or replayed, give the same bits.  No floating-point atomics.
//
// Dtypes follow numpy >= 2 (a float32 scalar combined with a Python number stays float32), as
// tests/loss_restatement.py states them; built with -ffp-contract=off so that every float32 step
// rounds like numpy's.
#include <math.h>

#include "dispatch.h"

#pragma clang fp contract(off)

namespace sfa {

namespace {

constexpr int kTgtThreads = 256;
constexpr int kTgtCellsPerThread = 4;
constexpr int kMaxObjects = 256;
constexpr int kMaxClasses = 16;

enum : int { kObjSkip = 0, kObjReal = 1, kObjIgnore = 2 };
enum : unsigned { kStatusIndex = 1u, kStatusClass = 2u };

struct TargetGeo {
  float min_x, max_x, min_y, max_y, min_z, max_z;  // the boundary as float32 (NEP 50 comparisons)
  float bound_x, bound_y;                          // f32(maxX - minX), f32(maxY - minY)
  int H, W, C, M;
  unsigned flip_lo, flip_hi;
};

// kitti_data_utils.py:176-197 on Python ints / floats (float64), then max(0, int(.)).
__device__ __forceinline__ int label_radius(double height, double width) {
  const double s = height + width, p = width * height;
  const double c1 = p * (1 - 0.7) / (1 + 0.7);
  const double r1 = (s + sqrt(s * s - 4 * c1)) / 2;
  const double b2 = 2 * s;
  const double c2 = (1 - 0.7) * width * height;
  const double r2 = (b2 + sqrt(b2 * b2 - 16 * c2)) / 2;
  const double b3 = -2 * 0.7 * s;
  const double c3 = (0.7 - 1) * width * height;
  const double r3 = (b3 + sqrt(b3 * b3 - 4 * (4 * 0.7) * c3)) / 2;
  double r = r1;  // Python min(): the first of the smallest
  if (r2 < r) r = r2;
  if (r3 < r) r = r3;
  if (!(r > 0)) return 0;
  return r < 1073741823.0 ? (int)r : 1073741823;
}

__global__ void __launch_bounds__(kTgtThreads)
    build_targets_kernel(const float* __restrict__ labels, const int64_t* __restrict__ offsets, int64_t total_rows,
                         TargetGeo g, float* __restrict__ hm, float* __restrict__ cen_offset,
                         float* __restrict__ direction, float* __restrict__ z_coor, float* __restrict__ dimension,
                         int64_t* __restrict__ indices, uint8_t* __restrict__ mask, uint32_t* __restrict__ status) {
  __shared__ int o_kind[kMaxObjects], o_cls[kMaxObjects], o_cx[kMaxObjects], o_cy[kMaxObjects], o_r[kMaxObjects];
  __shared__ double o_den[kMaxObjects];
  __shared__ unsigned s_flags;
  const int b = blockIdx.y, tid = threadIdx.x;
  const bool flipped = ((b < 32 ? g.flip_lo >> b : g.flip_hi >> (b - 32)) & 1u) != 0;
  int64_t r0 = offsets[b], r1 = offsets[b + 1];
  r0 = r0 < 0 ? 0 : (r0 > total_rows ? total_rows : r0);
  r1 = r1 < r0 ? r0 : (r1 > total_rows ? total_rows : r1);
  const int n = (int)(r1 - r0 < (int64_t)g.M ? r1 - r0 : (int64_t)g.M);  // min(len(labels), max_objects)
  if (tid == 0) s_flags = 0;
  __syncthreads();

  for (int k = tid; k < g.M; k += kTgtThreads) {
    int kind = kObjSkip, cls = 0, cxi = 0, cyi = 0, rad = 0;
    double den = 1.0;
    float off0 = 0.f, off1 = 0.f, dir0 = 0.f, dir1 = 0.f, zc = 0.f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
    int64_t index = 0;
    unsigned flags = 0;
    if (k < n) {
      const float* row = labels + (r0 + k) * 8;
      const float cf = row[0], x = row[1], y = row[2], z = row[3], h = row[4], w = row[5], l = row[6];
      const float yaw = -row[7];
      const bool inside = g.min_x <= x && x <= g.max_x && g.min_y <= y && y <= g.max_y && g.min_z <= z && z <= g.max_z;
      if (inside && !(h <= 0.f || w <= 0.f || l <= 0.f)) {
        // int(cls_id) truncates; a class the reference's indexing refuses (or a NaN) skips the row
        const bool cls_ok = cf > (float)(-g.C - 2) && cf < (float)g.C;
        if (!cls_ok) {
          flags |= kStatusClass;
        } else {
          cls = (int)cf;
          const float bbox_l = l / g.bound_x * (float)g.H;
          const float bbox_w = w / g.bound_y * (float)g.W;
          rad = label_radius(ceil((double)bbox_l), ceil((double)bbox_w));
          float cy = (x - g.min_x) / g.bound_x * (float)g.H;  // x --> y
          float cx = (y - g.min_y) / g.bound_y * (float)g.W;  // y --> x
          if (flipped) cx = (float)g.W - cx - 1.f;
          cxi = (int)cx;
          cyi = (int)cy;
          const double diameter = 2.0 * rad + 1.0, sigma = diameter / 6.0;
          den = 2 * sigma * sigma;
          if (cxi < 0 || cxi >= g.W || cyi < 0 || cyi >= g.H) flags |= kStatusIndex;
          if (cls < 0) {
            kind = kObjIgnore;
            cls = cls == -1 ? -1 : -cls - 2;
          } else {
            kind = kObjReal;
            index = (int64_t)(cyi * g.W + cxi);
            off0 = cx - (float)cxi;  // exact in either precision
            off1 = cy - (float)cyi;
            d0 = h;
            d1 = w;
            d2 = l;
            const float im = (float)sin((double)yaw);
            dir0 = flipped ? -im : im;
            dir1 = (float)cos((double)yaw);
            zc = z - g.min_z;
          }
        }
      }
    }
    o_kind[k] = kind;
    o_cls[k] = cls;
    o_cx[k] = cxi;
    o_cy[k] = cyi;
    o_r[k] = rad;
    o_den[k] = den;
    if (flags) atomicOr(&s_flags, flags);
    if (blockIdx.x == 0) {
      const size_t s = (size_t)b * g.M + k;
      cen_offset[s * 2] = off0;
      cen_offset[s * 2 + 1] = off1;
      direction[s * 2] = dir0;
      direction[s * 2 + 1] = dir1;
      z_coor[s] = zc;
      dimension[s * 3] = d0;
      dimension[s * 3 + 1] = d1;
      dimension[s * 3 + 2] = d2;
      indices[s] = index;
      mask[s] = kind == kObjReal ? 1 : 0;
    }
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) status[b] = s_flags;

  const int HW = g.H * g.W;
  const int64_t cells = (int64_t)g.C * HW;
  const float ignore_value = 0.9999f;
  float* out = hm + (size_t)b * cells;
  const int64_t first = (int64_t)blockIdx.x * (kTgtThreads * kTgtCellsPerThread) + tid;
#pragma unroll
  for (int j = 0; j < kTgtCellsPerThread; ++j) {
    const int64_t i = first + (int64_t)j * kTgtThreads;
    if (i >= cells) break;
    const int c = (int)(i / HW), p = (int)(i - (int64_t)c * HW);
    const int py = p / g.W, px = p - py * g.W;
    float v = 0.f;
    for (int k = 0; k < n; ++k) {
      const int kind = o_kind[k];
      if (kind == kObjSkip) continue;
      const int oc = o_cls[k];
      if (oc != c && !(kind == kObjIgnore && oc < 0)) continue;
      const int dx = px - o_cx[k], dy = py - o_cy[k], r = o_r[k];
      if (dx < -r || dx > r || dy < -r || dy > r) continue;
      const float gv = (float)exp(-((double)dx * dx + (double)dy * dy) / o_den[k]);
      v = gv > v ? gv : v;
      if (kind == kObjIgnore && dx == 0 && dy == 0) v = ignore_value;
    }
    out[i] = v;
  }
}

// ---------------------------------------------------------------- loss --
constexpr int kFocalThreads = 256;
constexpr int kFocalChunk = kFocalThreads * 16;  // cells per block: four float4 per thread
constexpr int kRowThreads = 256;

__device__ __forceinline__ float sigmoid_clamp_f(float x) {  // utils/torch_utils.py:44-45, as decode.hip
  const float s = 1.0f / (1.0f + expf(-x));
  return fminf(fmaxf(s, 1e-4f), 1.0f - 1e-4f);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Sum of one double per thread over the block, in a fixed order; valid in thread 0.
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* lds /*[THREADS / 64]*/) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) s += lds[w];
  }
  return s;
}

__device__ __forceinline__ void focal_term(float pred, float gt, int apply_sigmoid, double& pos, double& neg,
                                           double& npos) {
  const double p = (double)(apply_sigmoid ? sigmoid_clamp_f(pred) : pred);
  if (gt == 1.f) {
    const double q = 1 - p;
    pos += log(p) * (q * q);
    npos += 1;
  } else if (gt < 1.f) {
    const double w = 1 - (double)gt, w2 = w * w;
    neg += log1p(-p) * (p * p) * (w2 * w2);
  }
}

// partial[blockIdx.x * 3 + {0, 1, 2}] = pos, neg, num_pos of cells [blockIdx.x * kFocalChunk, ...)
template <bool VEC>
__global__ void __launch_bounds__(kFocalThreads)
    focal_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int64_t n, int apply_sigmoid,
                         double* __restrict__ partial) {
  __shared__ double lds[kFocalThreads / 64];
  double pos = 0, neg = 0, npos = 0;
  const int64_t base = (int64_t)blockIdx.x * kFocalChunk;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t i = base + ((int64_t)it * kFocalThreads + threadIdx.x) * 4;
    if (i >= n) break;
    if (VEC && i + 4 <= n) {
      const float4 p = *reinterpret_cast<const float4*>(pred + i);
      const float4 t = *reinterpret_cast<const float4*>(gt + i);
      focal_term(p.x, t.x, apply_sigmoid, pos, neg, npos);
      focal_term(p.y, t.y, apply_sigmoid, pos, neg, npos);
      focal_term(p.z, t.z, apply_sigmoid, pos, neg, npos);
      focal_term(p.w, t.w, apply_sigmoid, pos, neg, npos);
    } else {
      for (int j = 0; j < 4 && i + j < n; ++j) focal_term(pred[i + j], gt[i + j], apply_sigmoid, pos, neg, npos);
    }
  }
  pos = block_sum<kFocalThreads>(pos, lds);
  neg = block_sum<kFocalThreads>(neg, lds);
  npos = block_sum<kFocalThreads>(npos, lds);
  if (threadIdx.x == 0) {
    partial[(size_t)blockIdx.x * 3] = pos;
    partial[(size_t)blockIdx.x * 3 + 1] = neg;
    partial[(size_t)blockIdx.x * 3 + 2] = npos;
  }
}

struct LossMaps {
  const float *off, *dir, *z, *dim;          // predictions, NCHW
  const float *t_off, *t_dir, *t_z, *t_dim;  // targets, (B, M, c)
  const int64_t* ind;
  const uint8_t* mask;
};

// losses.py:116-125 with alpha 0.5, gamma 1.5, beta 1; bb = e^3 - 1
__device__ __forceinline__ double balanced_l1(double diff, double bb) {
  return diff < 1.0 ? 0.5 / bb * (bb * diff + 1) * log(bb * diff / 1.0 + 1) - 0.5 * diff
                    : 1.5 * diff + 1.5 / bb - 0.5 * 1.0;
}

// partial[blockIdx.x * 6 + {0..4}] = the cen_offset, dim, direction, z_coor sums and the mask sum of
// 256 slot rows; word [.. + 5] carries the block's status bits.
__global__ void __launch_bounds__(kRowThreads)
    rows_partial_kernel(LossMaps m, int B, int M, int64_t HW, int apply_sigmoid, double bb,
                        double* __restrict__ partial) {
  __shared__ double lds[kRowThreads / 64];
  __shared__ unsigned s_flags;
  if (threadIdx.x == 0) s_flags = 0;
  __syncthreads();
  double s_off = 0, s_dim = 0, s_dir = 0, s_z = 0, s_mask = 0;
  const int64_t row = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  if (row < (int64_t)B * M) {
    const double mk = (double)m.mask[row];
    if (mk != 0) {
      const int b = (int)(row / M);
      const int64_t idx = m.ind[row];
      if (idx < 0 || idx >= HW) {
        atomicOr(&s_flags, kStatusIndex);
      } else {
        s_mask = mk;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float pv = m.off[((size_t)b * 2 + c) * HW + idx];
          const double p = (double)(apply_sigmoid ? sigmoid_clamp_f(pv) : pv);
          s_off += fabs(p * mk - (double)m.t_off[row * 2 + c] * mk);
          s_dir += fabs((double)m.dir[((size_t)b * 2 + c) * HW + idx] * mk - (double)m.t_dir[row * 2 + c] * mk);
        }
        s_z = balanced_l1(fabs((double)m.z[(size_t)b * HW + idx] * mk - (double)m.t_z[row] * mk), bb);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          s_dim += balanced_l1(
              fabs((double)m.dim[((size_t)b * 3 + c) * HW + idx] * mk - (double)m.t_dim[row * 3 + c] * mk), bb);
      }
    }
  }
  s_off = block_sum<kRowThreads>(s_off, lds);
  s_dim = block_sum<kRowThreads>(s_dim, lds);
  s_dir = block_sum<kRowThreads>(s_dir, lds);
  s_z = block_sum<kRowThreads>(s_z, lds);
  s_mask = block_sum<kRowThreads>(s_mask, lds);
  if (threadIdx.x == 0) {
    double* o = partial + (size_t)blockIdx.x * 6;
    o[0] = s_off;
    o[1] = s_dim;
    o[2] = s_dir;
    o[3] = s_z;
    o[4] = s_mask;
    o[5] = (double)s_flags;
  }
}

// One block: thread t adds partials t, t + 256, ... in that order, then the block sum.
__global__ void __launch_bounds__(256)
    loss_fold_kernel(const double* __restrict__ focal, int n_focal, const double* __restrict__ rows, int n_rows,
                     float* __restrict__ loss, double* __restrict__ sums, uint32_t* __restrict__ status) {
  __shared__ double lds[4];
  double tot[8];
  double flags = 0;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    double v = 0;
    for (int i = threadIdx.x; i < n_focal; i += 256) v += focal[(size_t)i * 3 + q];
    tot[q] = block_sum<256>(v, lds);
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    double v = 0;
    for (int i = threadIdx.x; i < n_rows; i += 256) v += rows[(size_t)i * 6 + q];
    tot[3 + q] = block_sum<256>(v, lds);
  }
  for (int i = threadIdx.x; i < n_rows; i += 256) flags = fmax(flags, rows[(size_t)i * 6 + 5]);
  const unsigned any = __syncthreads_or(flags != 0);
  if (threadIdx.x != 0) return;
  const double pos = tot[0], neg = tot[1], npos = tot[2];
  const double hm = npos == 0 ? -neg : -(pos + neg) / npos;  // losses.py:65-68
  const double l_off = tot[3] / (tot[7] * 2 + 1e-4);         // mask.sum() over the expanded mask
  const double l_dim = tot[4] / (tot[7] * 3 + 1e-4);
  const double l_dir = tot[5] / (tot[7] * 2 + 1e-4);
  const double l_z = tot[6] / (tot[7] * 1 + 1e-4);
  loss[0] = (float)(hm + l_off + l_dim + l_dir + l_z);  // losses.py:150-152, unit weights
  loss[1] = (float)hm;
  loss[2] = (float)l_off;
  loss[3] = (float)l_dim;
  loss[4] = (float)l_dir;
  loss[5] = (float)l_z;
#pragma unroll
  for (int q = 0; q < 8; ++q) sums[q] = tot[q];
  *status = any ? kStatusIndex : 0u;
}

struct LossPlan {
  int64_t cells;
  int n_focal, n_rows;
  size_t rows_offset, bytes;
};

bool loss_plan(int B, int C, int H, int W, int M, LossPlan* p) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || M <= 0) return false;
  if (B > SFA_BEV_MAX_BATCH || C > kMaxClasses || M > kMaxObjects) return false;
  if ((int64_t)H * W > (int64_t)1 << 24) return false;
  p->cells = (int64_t)B * C * H * W;
  p->n_focal = (int)((p->cells + kFocalChunk - 1) / kFocalChunk);
  p->n_rows = (B * M + kRowThreads - 1) / kRowThreads;
  p->rows_offset = align_up((size_t)p->n_focal * 3 * sizeof(double), 256);
  p->bytes = p->rows_offset + align_up((size_t)p->n_rows * 6 * sizeof(double), 256);
  return true;
}

// ------------------------------------------------------------ loss gradient --
// d total / d (the five head maps), unit weights.  Three launches: gt == 1 is counted per 4096-cell
// chunk, one block folds the counts and the mask sum into the two scalars every gradient needs
// (the focal scale and the object count), and a gather pass writes every cell of the five maps.
// gather's backward is a scatter-add; here, as in build_targets_kernel, each thread owns cells and
// walks the frame's slot rows in slot order from LDS, so duplicates add up in a fixed order, cells
// no slot points at get 0.0, every output byte is written and there are no atomics.
constexpr int kGradThreads = 256;
constexpr int kGradPix = 4;                             // pixels per thread: one float4 per channel
constexpr int kGradTile = kGradThreads * kGradPix;      // pixels of one frame per block
constexpr size_t kGradScalarBytes = 256;                // workspace head: double {focal scale, mask sum}

template <bool VEC>
__global__ void __launch_bounds__(kFocalThreads)
    grad_count_kernel(const float* __restrict__ gt, int64_t n, uint32_t* __restrict__ counts) {
  __shared__ double lds[kFocalThreads / 64];
  int c = 0;
  const int64_t base = (int64_t)blockIdx.x * kFocalChunk;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t i = base + ((int64_t)it * kFocalThreads + threadIdx.x) * 4;
    if (i >= n) break;
    if (VEC && i + 4 <= n) {
      const float4 t = *reinterpret_cast<const float4*>(gt + i);
      c += (t.x == 1.f) + (t.y == 1.f) + (t.z == 1.f) + (t.w == 1.f);
    } else {
      for (int j = 0; j < 4 && i + j < n; ++j) c += gt[i + j] == 1.f;
    }
  }
  const double s = block_sum<kFocalThreads>((double)c, lds);  // integers: exact in any order
  if (threadIdx.x == 0) counts[blockIdx.x] = (uint32_t)s;
}

// One block.  scal[0] = -1 / num_pos (-1 when num_pos == 0), scal[1] = the mask sum over the slots
// whose index is inside the map, as sfa_compute_loss counts it.
__global__ void __launch_bounds__(256)
    grad_fold_kernel(const uint32_t* __restrict__ counts, int n_counts, const int64_t* __restrict__ ind,
                     const uint8_t* __restrict__ mask, int rows, int64_t HW, double* __restrict__ scal,
                     uint32_t* __restrict__ status) {
  __shared__ double lds[4];
  double npos = 0, msum = 0;
  bool bad = false;
  for (int i = threadIdx.x; i < n_counts; i += 256) npos += (double)counts[i];
  for (int r = threadIdx.x; r < rows; r += 256) {
    const unsigned mk = mask[r];
    if (mk == 0) continue;
    const int64_t idx = ind[r];
    if (idx < 0 || idx >= HW)
      bad = true;
    else
      msum += (double)mk;
  }
  npos = block_sum<256>(npos, lds);
  msum = block_sum<256>(msum, lds);
  const unsigned any = __syncthreads_or(bad);
  if (threadIdx.x != 0) return;
  scal[0] = npos == 0 ? -1.0 : -1.0 / npos;
  scal[1] = msum;
  *status = any ? kStatusIndex : 0u;
}

// _sigmoid's backward (utils/torch_utils.py:44-45): sigmoid' = s (1 - s), and clamp passes the
// gradient where min <= s <= max, both ends included.  s is sigmoid_clamp_f's float32 value.
__device__ __forceinline__ double sigmoid_chain(float x) {
  const float s = 1.0f / (1.0f + expf(-x));
  const double sd = (double)s;
  return (s >= 1e-4f && s <= 1.0f - 1e-4f) ? sd * (1 - sd) : 0.0;
}

// d hm_cen_loss / d pred of one cell (losses.py:44-69); k = -1 / num_pos
__device__ __forceinline__ float focal_grad(float pred, float gt, int apply_sigmoid, double k) {
  const double p = (double)(apply_sigmoid ? sigmoid_clamp_f(pred) : pred);
  double g = 0;
  if (gt == 1.f) {
    const double q = 1 - p;
    g = k * (q * q / p - 2 * q * log(p));
  } else if (gt < 1.f) {
    const double w = 1 - (double)gt, w2 = w * w;
    g = k * (w2 * w2) * (2 * p * log1p(-p) - p * p / (1 - p));
  }
  if (apply_sigmoid) g *= sigmoid_chain(pred);
  return (float)g;
}

__device__ __forceinline__ double sign_of(double d) { return d > 0 ? 1.0 : (d < 0 ? -1.0 : 0.0); }

struct GradMaps {
  float *hm, *off, *dir, *z, *dim;
};

// grid (ceil(HW / kGradTile), B).  Slot gradient columns: 0-1 cen_offset, 2-3 direction, 4 z_coor, 5-7 dim.
template <bool VEC>
__global__ void __launch_bounds__(kGradThreads)
    loss_grad_kernel(const float* __restrict__ hm, const float* __restrict__ t_hm, LossMaps m, GradMaps g, int C,
                     int M, int HW, int apply_sigmoid, double bb, const double* __restrict__ scal) {
  __shared__ double s_g[8][kMaxObjects];
  __shared__ int s_idx[kMaxObjects];
  const int b = blockIdx.y, tid = threadIdx.x;
  const double k = scal[0], msum = scal[1];
  const double den1 = msum * 1 + 1e-4, den2 = msum * 2 + 1e-4, den3 = msum * 3 + 1e-4;

  for (int s = tid; s < M; s += kGradThreads) {
    const int64_t row = (int64_t)b * M + s;
    const double mk = (double)m.mask[row];
    const int64_t idx = m.ind[row];
    const bool live = mk != 0 && idx >= 0 && idx < (int64_t)HW;
    double v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = 0;
    if (live) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float pv = m.off[((size_t)b * 2 + c) * HW + idx];
        const double p = (double)(apply_sigmoid ? sigmoid_clamp_f(pv) : pv);
        double go = sign_of(p * mk - (double)m.t_off[row * 2 + c] * mk) * mk / den2;
        if (apply_sigmoid) go *= sigmoid_chain(pv);
        v[c] = go;
        v[2 + c] =
            sign_of((double)m.dir[((size_t)b * 2 + c) * HW + idx] * mk - (double)m.t_dir[row * 2 + c] * mk) * mk / den2;
      }
      {
        const double d = (double)m.z[(size_t)b * HW + idx] * mk - (double)m.t_z[row] * mk, a = fabs(d);
        v[4] = sign_of(d) * mk * (a < 1.0 ? 0.5 * log(bb * a + 1) : 1.5) / den1;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double d = (double)m.dim[((size_t)b * 3 + c) * HW + idx] * mk - (double)m.t_dim[row * 3 + c] * mk;
        const double a = fabs(d);
        v[5 + c] = sign_of(d) * mk * (a < 1.0 ? 0.5 * log(bb * a + 1) : 1.5) / den3;
      }
    }
    s_idx[s] = live ? (int)idx : -1;
#pragma unroll
    for (int c = 0; c < 8; ++c) s_g[c][s] = v[c];
  }
  __syncthreads();

  const int p0 = ((int)blockIdx.x * kGradThreads + tid) * kGradPix;
  if (p0 >= HW) return;
  const int np = HW - p0 < kGradPix ? HW - p0 : kGradPix;

  // the focal gradient of this thread's pixels, class by class
  for (int c = 0; c < C; ++c) {
    const size_t o = ((size_t)b * C + c) * HW + p0;
    if (VEC && np == kGradPix) {
      const float4 p = *reinterpret_cast<const float4*>(hm + o);
      const float4 t = *reinterpret_cast<const float4*>(t_hm + o);
      float4 r;
      r.x = focal_grad(p.x, t.x, apply_sigmoid, k);
      r.y = focal_grad(p.y, t.y, apply_sigmoid, k);
      r.z = focal_grad(p.z, t.z, apply_sigmoid, k);
      r.w = focal_grad(p.w, t.w, apply_sigmoid, k);
      *reinterpret_cast<float4*>(g.hm + o) = r;
    } else {
      for (int j = 0; j < np; ++j) g.hm[o + j] = focal_grad(hm[o + j], t_hm[o + j], apply_sigmoid, k);
    }
  }

  // the regression heads: the slots of this frame that point at one of the pixels, in slot order
  double acc[kGradPix][8];
#pragma unroll
  for (int j = 0; j < kGradPix; ++j)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[j][c] = 0;
  for (int s = 0; s < M; ++s) {
    const unsigned rel = (unsigned)(s_idx[s] - p0);
    if (rel >= (unsigned)kGradPix) continue;
#pragma unroll
    for (int j = 0; j < kGradPix; ++j)
      if (rel == (unsigned)j) {
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[j][c] += s_g[c][s];
      }
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float* out = c < 2 ? g.off + ((size_t)b * 2 + c) * HW
                       : c < 4 ? g.dir + ((size_t)b * 2 + (c - 2)) * HW
                               : c < 5 ? g.z + (size_t)b * HW : g.dim + ((size_t)b * 3 + (c - 5)) * HW;
    if (VEC && np == kGradPix) {
      *reinterpret_cast<float4*>(out + p0) =
          make_float4((float)acc[0][c], (float)acc[1][c], (float)acc[2][c], (float)acc[3][c]);
    } else {
#pragma unroll
      for (int j = 0; j < kGradPix; ++j)
        if (j < np) out[p0 + j] = (float)acc[j][c];
    }
  }
}

struct GradPlan {
  int64_t cells;
  int n_counts;
  size_t bytes;
};

bool grad_plan(int B, int C, int H, int W, int M, GradPlan* p) {
  LossPlan lp;
  if (!loss_plan(B, C, H, W, M, &lp)) return false;
  p->cells = lp.cells;
  p->n_counts = lp.n_focal;
  p->bytes = kGradScalarBytes + align_up((size_t)p->n_counts * sizeof(uint32_t), 256);
  return true;
}

}  // namespace

}  // namespace sfa

using namespace sfa;

extern "C" int sfa_build_targets(const float* labels, const int64_t* frame_offsets, int64_t total_rows, int batch,
                                 const sfa_target_params* params, float* hm_cen, float* cen_offset,
                                 float* direction, float* z_coor, float* dim, int64_t* indices_center,
                                 uint8_t* obj_mask, uint32_t* status, void* stream) {
  SFA_CHECK_ARG(params, "build_targets: null params");
  const sfa_target_params& p = *params;
  SFA_CHECK_ARG(batch > 0 && p.num_classes > 0 && p.hm_h > 0 && p.hm_w > 0,
                "build_targets: batch %d, classes %d, map %d x %d must be positive", batch, p.num_classes, p.hm_h,
                p.hm_w);
  SFA_CHECK_ARG(batch <= 64, "build_targets: batch %d > 64 (one h-flip bit per frame)", batch);
  SFA_CHECK_ARG(p.num_classes <= kMaxClasses, "build_targets: num_classes %d > %d", p.num_classes, kMaxClasses);
  SFA_CHECK_ARG(p.max_objects >= 1 && p.max_objects <= kMaxObjects, "build_targets: max_objects %d outside 1..%d",
                p.max_objects, kMaxObjects);
  SFA_CHECK_ARG((int64_t)p.hm_h * p.hm_w <= (int64_t)1 << 24, "build_targets: map %d x %d above 2^24 cells", p.hm_h,
                p.hm_w);
  for (int i = 0; i < 6; ++i) SFA_CHECK_ARG(p.reserved[i] == 0, "build_targets: reserved words must be zero");
  SFA_CHECK_ARG(total_rows >= 0, "build_targets: negative row count");
  SFA_CHECK_ARG(labels && frame_offsets && hm_cen && cen_offset && direction && z_coor && dim && indices_center &&
                    obj_mask && status,
                "build_targets: null buffer");
  TargetGeo g;
  g.min_x = (float)p.boundary[0];
  g.max_x = (float)p.boundary[1];
  g.min_y = (float)p.boundary[2];
  g.max_y = (float)p.boundary[3];
  g.min_z = (float)p.boundary[4];
  g.max_z = (float)p.boundary[5];
  g.bound_x = (float)(p.boundary[1] - p.boundary[0]);
  g.bound_y = (float)(p.boundary[3] - p.boundary[2]);
  g.H = p.hm_h;
  g.W = p.hm_w;
  g.C = p.num_classes;
  g.M = p.max_objects;
  g.flip_lo = p.hflip_mask_lo;
  g.flip_hi = p.hflip_mask_hi;
  const int64_t cells = (int64_t)g.C * g.H * g.W;
  const int per_block = kTgtThreads * kTgtCellsPerThread;
  const dim3 grid((unsigned)((cells + per_block - 1) / per_block), (unsigned)batch);
  return launch({grid, dim3(kTgtThreads), reinterpret_cast<hipStream_t>(stream)}, build_targets_kernel, labels,
                frame_offsets, total_rows, g, hm_cen, cen_offset, direction, z_coor, dim, indices_center, obj_mask,
                status);
}

extern "C" size_t sfa_compute_loss_workspace_size(int batch, int num_classes, int height, int width,
                                                  int max_objects) {
  LossPlan p;
  return loss_plan(batch, num_classes, height, width, max_objects, &p) ? p.bytes : 0;
}

// The head maps, targets and slot rows both loss entries take.
struct LossInputs {
  const float *hm_cen, *cen_offset, *direction, *z_coor, *dim;
  const float *t_hm_cen, *t_cen_offset, *t_direction, *t_z_coor, *t_dim;
  const int64_t* indices_center;
  const uint8_t* obj_mask;
  LossMaps maps() const {
    return {cen_offset, direction, z_coor, dim, t_cen_offset, t_direction, t_z_coor, t_dim, indices_center, obj_mask};
  }
};

// The checks both entries share: the shape (plan_ok: the entry's plan accepted it), the buffers
// (outputs_ok: the entry's own ones) and the workspace against the plan's size.
static int loss_check(const char* who, bool plan_ok, const LossInputs& in, bool outputs_ok, int batch, int num_classes,
                      int height, int width, int max_objects, const void* workspace, size_t workspace_bytes,
                      size_t need) {
  SFA_CHECK_ARG(plan_ok, "%s: batch %d (1..64), classes %d (1..%d), map %d x %d, max_objects %d (1..%d)", who, batch,
                num_classes, kMaxClasses, height, width, max_objects, kMaxObjects);
  SFA_CHECK_ARG(in.hm_cen && in.cen_offset && in.direction && in.z_coor && in.dim && in.t_hm_cen && in.t_cen_offset &&
                    in.t_direction && in.t_z_coor && in.t_dim && in.indices_center && in.obj_mask && outputs_ok &&
                    workspace,
                "%s: null buffer", who);
  SFA_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: workspace not 8-byte aligned", who);
  if (workspace_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return SFA_E_WORKSPACE;
  }
  return SFA_OK;
}

extern "C" int sfa_compute_loss(const float* hm_cen, const float* cen_offset, const float* direction,
                                const float* z_coor, const float* dim, const float* t_hm_cen,
                                const float* t_cen_offset, const float* t_direction, const float* t_z_coor,
                                const float* t_dim, const int64_t* indices_center, const uint8_t* obj_mask, int batch,
                                int num_classes, int height, int width, int max_objects, int apply_sigmoid,
                                float* loss, double* sums, uint32_t* status, void* workspace, size_t workspace_bytes,
                                void* stream) {
  const LossInputs in{hm_cen,   cen_offset,   direction,   z_coor,   dim,   //
                      t_hm_cen, t_cen_offset, t_direction, t_z_coor, t_dim, indices_center, obj_mask};
  LossPlan p{};
  const bool plan_ok = loss_plan(batch, num_classes, height, width, max_objects, &p);
  if (int rc = loss_check("compute_loss", plan_ok, in, loss && sums && status, batch, num_classes, height, width,
                          max_objects, workspace, workspace_bytes, p.bytes))
    return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* focal = reinterpret_cast<double*>(workspace);
  double* rows = reinterpret_cast<double*>(static_cast<char*>(workspace) + p.rows_offset);
  const int sig = apply_sigmoid ? 1 : 0;
  const bool vec = (reinterpret_cast<uintptr_t>(hm_cen) | reinterpret_cast<uintptr_t>(t_hm_cen)) % 16 == 0;
  if (int rc = with_bool(vec, [&](auto VEC) {
        return launch({dim3(p.n_focal), dim3(kFocalThreads), st}, focal_partial_kernel<VEC.value>, hm_cen, t_hm_cen,
                      p.cells, sig, focal);
      }))
    return rc;
  if (int rc = launch({dim3(p.n_rows), dim3(kRowThreads), st}, rows_partial_kernel, in.maps(), batch, max_objects,
                      (int64_t)height * width, sig, exp(1.5 / 0.5) - 1, rows))
    return rc;
  return launch({dim3(1), dim3(256), st}, loss_fold_kernel, focal, p.n_focal, rows, p.n_rows, loss, sums, status);
}

extern "C" size_t sfa_compute_loss_grad_workspace_size(int batch, int num_classes, int height, int width,
                                                       int max_objects) {
  GradPlan p;
  return grad_plan(batch, num_classes, height, width, max_objects, &p) ? p.bytes : 0;
}

extern "C" int sfa_compute_loss_grad(const float* hm_cen, const float* cen_offset, const float* direction,
                                     const float* z_coor, const float* dim, const float* t_hm_cen,
                                     const float* t_cen_offset, const float* t_direction, const float* t_z_coor,
                                     const float* t_dim, const int64_t* indices_center, const uint8_t* obj_mask,
                                     int batch, int num_classes, int height, int width, int max_objects,
                                     int apply_sigmoid, float* g_hm_cen, float* g_cen_offset, float* g_direction,
                                     float* g_z_coor, float* g_dim, uint32_t* status, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  const LossInputs in{hm_cen,   cen_offset,   direction,   z_coor,   dim,   //
                      t_hm_cen, t_cen_offset, t_direction, t_z_coor, t_dim, indices_center, obj_mask};
  GradPlan p{};
  const bool plan_ok = grad_plan(batch, num_classes, height, width, max_objects, &p);
  if (int rc = loss_check("compute_loss_grad", plan_ok, in,
                          g_hm_cen && g_cen_offset && g_direction && g_z_coor && g_dim && status, batch, num_classes,
                          height, width, max_objects, workspace, workspace_bytes, p.bytes))
    return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* scal = reinterpret_cast<double*>(workspace);
  uint32_t* counts = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + kGradScalarBytes);
  const int HW = height * width;
  if (int rc = with_bool(reinterpret_cast<uintptr_t>(t_hm_cen) % 16 == 0, [&](auto VEC) {
        return launch({dim3(p.n_counts), dim3(kFocalThreads), st}, grad_count_kernel<VEC.value>, t_hm_cen, p.cells,
                      counts);
      }))
    return rc;
  if (int rc = launch({dim3(1), dim3(256), st}, grad_fold_kernel, counts, p.n_counts, indices_center, obj_mask,
                      batch * max_objects, (int64_t)HW, scal, status))
    return rc;
  const GradMaps g{g_hm_cen, g_cen_offset, g_direction, g_z_coor, g_dim};
  // 128-bit loads and stores need every channel plane 16-byte aligned: the bases and H*W % 4 == 0
  const uintptr_t bases = reinterpret_cast<uintptr_t>(hm_cen) | reinterpret_cast<uintptr_t>(t_hm_cen) |
                          reinterpret_cast<uintptr_t>(g_hm_cen) | reinterpret_cast<uintptr_t>(g_cen_offset) |
                          reinterpret_cast<uintptr_t>(g_direction) | reinterpret_cast<uintptr_t>(g_z_coor) |
                          reinterpret_cast<uintptr_t>(g_dim);
  const dim3 grid((unsigned)((HW + kGradTile - 1) / kGradTile), (unsigned)batch);
  return with_bool(bases % 16 == 0 && HW % 4 == 0, [&](auto VEC) {
    return launch({grid, dim3(kGradThreads), st}, loss_grad_kernel<VEC.value>, hm_cen, t_hm_cen, in.maps(), g,
                  num_classes, max_objects, HW, apply_sigmoid ? 1 : 0, exp(1.5 / 0.5) - 1, scal);
  });
}
