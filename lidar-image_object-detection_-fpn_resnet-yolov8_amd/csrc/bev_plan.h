// Scratch plans of the two voxelisers (bev.hip, bev_argo.hip): which path a call takes and where
// every region of the caller's scratch lies.  Plain C++ (no HIP), so the plans can be compiled and
// checked on their own (tools/bev_plan_check.cpp).
//
// The rule both follow: areas that must be zero between calls are placed by the scratch's size alone,
// the record regions (written before they are read, left dirty) lie after them, so calls of any batch
// that share a scratch never put records into another call's zero area.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/sfa_hip.h"

namespace sfa {

struct Region {
  size_t off, bytes;  // within the scratch
};

inline size_t bev_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------- KITTI --
constexpr int kBevH = 608;
constexpr int kBevW = 608;
constexpr int kBevCells = kBevH * kBevW;
constexpr int kStripRows = 8;                 // binned path: 8-row strips
constexpr int kStrips = kBevH / kStripRows;   // 76
constexpr int kBlkPts = 1024;                 // blocked path: points (records) of one region
constexpr int blk_strips(int sr) { return kBevH / sr; }                  // 152 / 76
constexpr int blk_max_regions(int sr) { return sr == 8 ? 2048 : 1024; }  // regions of one frame a strip block indexes

// atomic path: keys + counts per cell; the binned and blocked paths get as much again after them
// (12 B per cell of room: ~277 k 16-byte records per frame)
inline size_t bev_atomic_bytes(int batch) {
  return bev_align_up((size_t)batch * kBevCells * sizeof(unsigned long long), 256) +
         bev_align_up((size_t)batch * kBevCells * sizeof(unsigned), 256);
}
inline size_t bev_scratch_size(int batch) { return batch <= 0 ? 0 : 2 * bev_atomic_bytes(batch); }

// The layout is fixed by the scratch's CAPACITY (the largest batch it was sized for), never by the
// batch of the call.  A layout by the call's batch let a small-batch call's records land inside a
// later larger call's zero areas.
inline int bev_capacity_batch(size_t scratch_bytes) {
  int cap = 0;
  while (cap < SFA_BEV_MAX_BATCH && bev_scratch_size(cap + 1) <= scratch_bytes) ++cap;
  return cap;
}

enum class BevPath { kBlocked4, kBlocked8, kBinned, kAtomic };

struct BevPlan {
  BevPath path;
  int cap;                                     // frames the scratch holds
  Region keys, counts;                         // atomic path: per cell, zero between calls
  Region bin_count, bin_offset, bin_cursor;    // binned path: per (frame, strip), zero between calls
  Region blk_rec, blk_tab;                     // blocked path: 8-B records, strip-major table (dirty)
  Region bin_rec;                              // binned path: 16-B records (dirty)
  int blk0[SFA_BEV_MAX_BATCH + 1];             // first region of frame b: exclusive sum of ceil(n / 1024)
  int nblk_total;
};

// The paths in the order they are tried: blocked (SR 4, or SR 8 with SFA_BEV_STRIP8) when no frame
// has more regions than a strip block indexes and records + table fit after the binned counters;
// binned when the batch's points fit as 16-B records; else atomic.  frame_offsets: batch + 1 monotone
// values, every frame below 2^32 - 1 points; batch <= the scratch's capacity (checked by the caller).
inline BevPlan bev_plan(size_t scratch_bytes, int batch, const int64_t* frame_offsets, int flags) {
  BevPlan p{};
  p.cap = bev_capacity_batch(scratch_bytes);
  const size_t half = bev_atomic_bytes(p.cap);
  const size_t key_bytes = (size_t)p.cap * kBevCells * sizeof(unsigned long long);
  p.keys = {0, key_bytes};
  p.counts = {bev_align_up(key_bytes, 256), (size_t)p.cap * kBevCells * sizeof(unsigned)};
  const size_t ctr = (size_t)p.cap * kStrips * sizeof(unsigned), ctr_al = bev_align_up(ctr, 256);
  p.bin_count = {half, ctr};
  p.bin_offset = {half + ctr_al, ctr};
  p.bin_cursor = {half + 2 * ctr_al, ctr};

  const int sr = (flags & SFA_BEV_STRIP8) ? 8 : 4;
  int64_t nblk = 0;
  int max_regions = 0;
  for (int b = 0; b < batch; ++b) {
    p.blk0[b] = (int)nblk;
    nblk += (frame_offsets[b + 1] - frame_offsets[b] + kBlkPts - 1) / kBlkPts;
    if ((int)nblk - p.blk0[b] > max_regions) max_regions = (int)nblk - p.blk0[b];
  }
  p.blk0[batch] = p.nblk_total = (int)nblk;
  const size_t rec_bytes = (size_t)nblk * kBlkPts * 8, rec_al = bev_align_up(rec_bytes, 256);
  const size_t tab_bytes = (size_t)nblk * blk_strips(sr) * sizeof(unsigned);
  const bool force_atomic = (flags & SFA_BEV_FORCE_ATOMIC) != 0;
  if (!force_atomic && !(flags & SFA_BEV_FORCE_BINNED) && max_regions <= blk_max_regions(sr) &&
      3 * ctr_al + rec_al + tab_bytes <= half) {
    p.path = sr == 8 ? BevPath::kBlocked8 : BevPath::kBlocked4;
    p.blk_rec = {half + 3 * ctr_al, rec_bytes};
    p.blk_tab = {half + 3 * ctr_al + rec_al, tab_bytes};
    return p;
  }
  const int64_t total = frame_offsets[batch] - frame_offsets[0];
  if (!force_atomic && 3 * ctr_al < half && (uint64_t)total <= (uint64_t)((half - 3 * ctr_al) / 16) &&
      total < (int64_t)0xffffffff) {
    p.path = BevPath::kBinned;
    p.bin_rec = {half + 3 * ctr_al, (size_t)total * 16};
    return p;
  }
  p.path = BevPath::kAtomic;
  return p;
}

// --------------------------------------------------------------- Argoverse --
constexpr int kArgoMaxDim = SFA_ARGO_BEV_MAX_DIM;  // H, W <= 2048
constexpr int kArgoStripCells = 4096;              // cells of a strip at most: 3 LDS words each, 48 KiB
constexpr int kArgoMaxStripRows = 8;
constexpr int kArgoMaxStrips = 1024;               // H <= 2048 and SR >= 2 whenever W <= 2048
constexpr int kArgoBlkPts = 1024;
constexpr int kArgoMaxRegions = 1024;     // regions of one frame a strip block indexes (1 Mi points)
constexpr size_t kArgoHeaderBytes = 256;  // the frames' intensity maxima, SFA_BEV_MAX_BATCH words
static_assert(SFA_BEV_MAX_BATCH * sizeof(unsigned) <= kArgoHeaderBytes, "header");

inline size_t argo_atomic_bytes(int batch, int H, int W) {
  return kArgoHeaderBytes + bev_align_up((size_t)batch * H * W * 3 * sizeof(unsigned), 256);
}
// 0 for a batch or a map out of range
inline size_t argo_scratch_size(int batch, int H, int W) {
  if (batch < 1 || batch > SFA_BEV_MAX_BATCH || H < 1 || H > kArgoMaxDim || W < 1 || W > kArgoMaxDim) return 0;
  return 2 * argo_atomic_bytes(batch, H, W);
}

struct ArgoPlan {
  bool records;            // the record path; false: the atomic path
  int strip_rows, strips;  // SR, ceil(H / SR)
  size_t rec_base;         // the scratch's second half: where the dirty regions start
  Region fmax, cells3;     // the frames' maxima and the atomic path's cells: zero between calls
  Region zi, cell, tab;    // record path: {z, intensity} bits, cell within the strip, strip-major table
  int blk0[SFA_BEV_MAX_BATCH + 1];
  int nblk_total;
};

// First half: the frames' maximum words + the atomic path's cells; second half: the record path's
// regions and table.  The halves are split by the scratch's size alone, so calls of any batch and any
// map size that the scratch holds may share it.  scratch_bytes >= argo_scratch_size(batch, H, W)
// (checked by the caller).
inline ArgoPlan argo_plan(size_t scratch_bytes, int batch, const int64_t* frame_offsets, int H, int W,
                          bool force_atomic) {
  ArgoPlan p{};
  int sr = kArgoStripCells / W < kArgoMaxStripRows ? kArgoStripCells / W : kArgoMaxStripRows;
  if (H < sr) sr = H;
  p.strip_rows = sr < 1 ? 1 : sr;
  p.strips = (H + p.strip_rows - 1) / p.strip_rows;
  p.fmax = {0, (size_t)batch * sizeof(unsigned)};
  p.cells3 = {kArgoHeaderBytes, (size_t)batch * H * W * 3 * sizeof(unsigned)};
  p.rec_base = (scratch_bytes / 2) & ~(size_t)255;  // >= the atomic area's end
  int64_t nblk = 0, max_regions = 0;
  for (int b = 0; b < batch; ++b) {
    p.blk0[b] = (int)(nblk < INT32_MAX ? nblk : INT32_MAX);
    const int64_t r = (frame_offsets[b + 1] - frame_offsets[b] + kArgoBlkPts - 1) / kArgoBlkPts;
    nblk += r;
    if (r > max_regions) max_regions = r;
  }
  p.blk0[batch] = p.nblk_total = (int)nblk;
  const size_t zi_bytes = (size_t)nblk * kArgoBlkPts * 8;
  const size_t cell_bytes = (size_t)nblk * kArgoBlkPts * sizeof(unsigned short);
  const size_t tab_bytes = (size_t)nblk * p.strips * sizeof(unsigned);
  p.records = !force_atomic && max_regions <= kArgoMaxRegions && p.strips <= kArgoMaxStrips &&
              zi_bytes + cell_bytes + tab_bytes <= scratch_bytes - p.rec_base;
  if (p.records) {
    p.zi = {p.rec_base, zi_bytes};
    p.cell = {p.rec_base + zi_bytes, cell_bytes};
    p.tab = {p.rec_base + zi_bytes + cell_bytes, tab_bytes};
  }
  return p;
}

}  // namespace sfa
