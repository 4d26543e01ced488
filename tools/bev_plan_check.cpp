// Stand-alone check of the voxelisers' scratch plans (csrc/bev_plan.h), host only: for every
// capacity, batch, mix of frame sizes and flag set, the zero areas sit where the capacity alone puts
// them, no dirty region touches them, everything ends inside the scratch, and the path is the one
// the limits dictate.  Build with a sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/bev_plan_check.cpp -o /tmp/bev_plan_check
#include <cstdio>
#include <vector>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/bev_plan.h"

using namespace sfa;

static int bad = 0;
#define EXPECT(cond, ...)                                     \
  do {                                                        \
    if (!(cond)) {                                            \
      if (++bad <= 20) std::printf("FAIL " __VA_ARGS__), std::printf(": %s\n", #cond); \
    }                                                         \
  } while (0)

static bool disjoint(const Region& a, const Region& b) {
  return a.bytes == 0 || b.bytes == 0 || a.off + a.bytes <= b.off || b.off + b.bytes <= a.off;
}

static std::vector<int64_t> offsets(const std::vector<int64_t>& n, int64_t first = 0) {
  std::vector<int64_t> o{first};
  for (int64_t v : n) o.push_back(o.back() + v);
  return o;
}

static BevPlan kitti(int cap, const std::vector<int64_t>& n, int flags, size_t extra = 0) {
  return bev_plan(bev_scratch_size(cap) + extra, (int)n.size(), offsets(n, 7).data(), flags);
}

// ------------------------------------------------------------------- KITTI --
static void check_kitti(int cap, const std::vector<int64_t>& n, const int64_t* off, const BevPlan& ref, int flags,
                        size_t extra) {
  const int batch = (int)n.size();
  const size_t scratch = bev_scratch_size(cap) + extra;
  const BevPlan p = bev_plan(scratch, batch, off, flags);
  EXPECT(p.cap == cap, "cap %d batch %d flags %d", cap, batch, flags);
  const Region* zero[] = {&p.keys, &p.counts, &p.bin_count, &p.bin_offset, &p.bin_cursor};
  const Region* zref[] = {&ref.keys, &ref.counts, &ref.bin_count, &ref.bin_offset, &ref.bin_cursor};
  const Region* dirty[] = {&p.blk_rec, &p.blk_tab, &p.bin_rec};
  for (int i = 0; i < 5; ++i) {
    EXPECT(zero[i]->off == zref[i]->off && zero[i]->bytes == zref[i]->bytes, "zero area %d cap %d batch %d", i, cap, batch);
    EXPECT(zero[i]->off % 256 == 0 && zero[i]->off + zero[i]->bytes <= scratch, "zero area %d cap %d", i, cap);
    for (int j = 0; j < i; ++j) EXPECT(disjoint(*zero[i], *zero[j]), "zero areas %d %d cap %d", i, j, cap);
    for (const Region* d : dirty) EXPECT(disjoint(*zero[i], *d), "dirty in zero area %d cap %d batch %d flags %d", i, cap, batch, flags);
  }
  // what the kernels touch of the zero areas lies inside them
  EXPECT(p.keys.bytes >= (size_t)batch * kBevCells * 8 && p.counts.bytes >= (size_t)batch * kBevCells * 4 &&
             p.bin_count.bytes >= (size_t)batch * kStrips * 4,
         "zero areas hold the batch, cap %d batch %d", cap, batch);
  for (const Region* d : dirty) EXPECT(d->off % 256 == 0 && d->off + d->bytes <= scratch, "dirty region cap %d batch %d flags %d", cap, batch, flags);
  EXPECT(disjoint(p.blk_rec, p.blk_tab), "records / table cap %d", cap);
  int64_t sum = 0, total = 0, max_regions = 0;
  for (int b = 0; b < batch; ++b) {
    EXPECT(p.blk0[b] == sum, "blk0[%d] cap %d", b, cap);
    const int64_t r = (n[b] + kBlkPts - 1) / kBlkPts;
    sum += r;
    total += n[b];
    if (r > max_regions) max_regions = r;
  }
  EXPECT(p.blk0[batch] == sum && p.nblk_total == sum, "region total cap %d", cap);
  const bool blocked = p.path == BevPath::kBlocked4 || p.path == BevPath::kBlocked8;
  if (blocked) {
    const int sr = p.path == BevPath::kBlocked8 ? 8 : 4;
    EXPECT(max_regions <= blk_max_regions(sr), "frame above max_regions cap %d", cap);
    EXPECT(p.blk_rec.bytes == (size_t)sum * kBlkPts * 8 && p.blk_tab.bytes == (size_t)sum * blk_strips(sr) * 4, "blocked sizes cap %d", cap);
    EXPECT(((flags & SFA_BEV_STRIP8) != 0) == (sr == 8), "strip rows by flag");
    EXPECT(!(flags & (SFA_BEV_FORCE_ATOMIC | SFA_BEV_FORCE_BINNED)), "blocked although forced");
  } else {
    EXPECT(p.blk_rec.bytes == 0 && p.blk_tab.bytes == 0, "blocked regions on another path");
  }
  if (p.path == BevPath::kBinned) {
    EXPECT(p.bin_rec.bytes == (size_t)total * 16 && p.bin_rec.off % 16 == 0, "binned records cap %d", cap);
    EXPECT(!(flags & SFA_BEV_FORCE_ATOMIC), "binned although atomic forced");
  } else {
    EXPECT(p.bin_rec.bytes == 0, "binned records on another path");
  }
  if (flags & SFA_BEV_FORCE_ATOMIC) EXPECT(p.path == BevPath::kAtomic, "atomic not forced");
}

static void kitti_known_answers() {
  // One frame's atomic area is 608 * 608 * (8 + 4) = 4,435,968 B (both parts multiples of 256), so a
  // scratch of capacity c has c * 4,435,968 B after the zero areas' first half.  The binned counters
  // take 3 * align256(c * 76 * 4) of it.  A region is 1024 records of 8 B; a table row 152 (SR 4) or
  // 76 (SR 8) words per region; a binned record 16 B.
  const int64_t k130 = 132880;
  // capacity 16, 16 x 132,880: 130 regions a frame (<= 1024), 2080 in all; 2080 * 8192 = 17,039,360 B of
  // records + 2080 * 152 * 4 = 1,264,640 B of table + 3 * 4864 = 14,592 B of counters = 18,318,592
  // <= 16 * 4,435,968 = 70,975,488: blocked SR 4.
  EXPECT(kitti(16, std::vector<int64_t>(16, k130), 0).path == BevPath::kBlocked4, "known: 16 x 132,880");
  // capacity 1, 400,000: 391 regions; 391 * 8192 = 3,203,072 + 391 * 152 * 4 = 237,728 + 3 * 512 = 1,536
  // = 3,442,336 <= 4,435,968: blocked.
  EXPECT(kitti(1, {400000}, 0).path == BevPath::kBlocked4, "known: 400,000 at capacity 1");
  // capacity 1, 600,000: 586 regions need 4,800,512 B of records > 4,435,968: not blocked; the binned
  // room is (4,435,968 - 1,536) / 16 = 277,152 records < 600,000: atomic.
  EXPECT(kitti(1, {600000}, 0).path == BevPath::kAtomic, "known: 600,000 at capacity 1");
  EXPECT(kitti(1, {277152}, SFA_BEV_FORCE_BINNED).path == BevPath::kBinned, "known: binned room, last that fits");
  EXPECT(kitti(1, {277153}, SFA_BEV_FORCE_BINNED).path == BevPath::kAtomic, "known: binned room, first that does not");
  // capacity 8, [132,880, 1,200,000, 132,880]: 1,200,000 points are 1172 regions > 1024: not blocked;
  // 1,465,760 records <= (8 * 4,435,968 - 3 * 2,560) / 16 = 2,217,504: binned.
  EXPECT(kitti(8, {k130, 1200000, k130}, 0).path == BevPath::kBinned, "known: three-frame batch");
  // forced binned, 400,000 > 277,152 records at capacity 1: atomic.
  EXPECT(kitti(1, {400000}, SFA_BEV_FORCE_BINNED).path == BevPath::kAtomic, "known: forced binned, no room");
  // SFA_BEV_STRIP8, 1,500,000 points: 1465 regions (<= 2048); 1465 * 8192 = 12,001,280 + 1465 * 76 * 4 =
  // 445,360 B.  Capacity 3: + 3 * 1,024 = 12,449,712 <= 13,307,904: blocked SR 8.  Capacity 2:
  // 8,871,936 B do not hold the records, and (8,871,936 - 2,304) / 16 = 554,352 < 1,500,000: atomic.
  // Without the flag 1465 regions > 1024, and capacity 4 has room for 1,108,752 binned records: atomic.
  EXPECT(kitti(3, {1500000}, SFA_BEV_STRIP8).path == BevPath::kBlocked8, "known: strip8 at capacity 3");
  EXPECT(kitti(2, {1500000}, SFA_BEV_STRIP8).path == BevPath::kAtomic, "known: strip8 at capacity 2");
  EXPECT(kitti(4, {1500000}, 0).path == BevPath::kAtomic, "known: 1.5 M without strip8");
  // capacity: a scratch one byte short of c + 1 frames holds c
  for (int c = 1; c < SFA_BEV_MAX_BATCH; ++c)
    EXPECT(bev_capacity_batch(bev_scratch_size(c + 1) - 1) == c && bev_capacity_batch(bev_scratch_size(c)) == c, "capacity %d", c);
  EXPECT(bev_capacity_batch(0) == 0 && bev_capacity_batch(bev_scratch_size(64) * 2) == 64 && bev_scratch_size(0) == 0, "capacity ends");
}

// --------------------------------------------------------------- Argoverse --
static void check_argo(int batch_sized, int H, int W, const std::vector<int64_t>& n, bool force, size_t extra) {
  const int batch = (int)n.size();
  const size_t scratch = argo_scratch_size(batch_sized, H, W) + extra;
  const ArgoPlan p = argo_plan(scratch, batch, offsets(n, 3).data(), H, W, force);
  EXPECT(p.rec_base == ((scratch / 2) & ~(size_t)255) && p.rec_base % 256 == 0, "argo halves %d x %d", H, W);
  EXPECT(p.fmax.off == 0 && p.fmax.bytes <= kArgoHeaderBytes && p.cells3.off == kArgoHeaderBytes, "argo zero areas %d x %d", H, W);
  EXPECT(p.cells3.off + p.cells3.bytes <= p.rec_base, "argo cells past the first half %d x %d batch %d", H, W, batch);
  EXPECT(p.strip_rows >= 1 && p.strip_rows <= kArgoMaxStripRows && (p.strip_rows == 1 || p.strip_rows * W <= kArgoStripCells) &&
             p.strip_rows * W <= kArgoStripCells && p.strips * p.strip_rows >= H && (p.strips - 1) * p.strip_rows < H,
         "argo strips %d x %d", H, W);
  int64_t sum = 0, max_regions = 0;
  for (int b = 0; b < batch; ++b) {
    EXPECT(p.blk0[b] == sum, "argo blk0[%d]", b);
    const int64_t r = (n[b] + kArgoBlkPts - 1) / kArgoBlkPts;
    sum += r;
    if (r > max_regions) max_regions = r;
  }
  EXPECT(p.blk0[batch] == sum && p.nblk_total == sum, "argo region total");
  if (p.records) {
    EXPECT(!force && max_regions <= kArgoMaxRegions && p.strips <= kArgoMaxStrips, "argo records outside the limits");
    EXPECT(p.zi.off == p.rec_base && p.zi.off % 8 == 0 && p.cell.off == p.zi.off + p.zi.bytes && p.cell.off % 2 == 0 &&
               p.tab.off == p.cell.off + p.cell.bytes && p.tab.off % 4 == 0 && p.tab.off + p.tab.bytes <= scratch,
           "argo record regions %d x %d batch %d", H, W, batch);
    EXPECT(p.zi.bytes == (size_t)sum * kArgoBlkPts * 8 && p.cell.bytes == (size_t)sum * kArgoBlkPts * 2 &&
               p.tab.bytes == (size_t)sum * p.strips * 4,
           "argo record sizes");
    const Region* dirty[] = {&p.zi, &p.cell, &p.tab};
    for (const Region* d : dirty) EXPECT(disjoint(*d, p.fmax) && disjoint(*d, p.cells3), "argo dirty in zero area %d x %d", H, W);
  } else {
    EXPECT(p.zi.bytes == 0 && p.cell.bytes == 0 && p.tab.bytes == 0, "argo regions on the atomic path");
  }
}

static void argo_known_answers() {
  auto path = [](int batch_sized, int H, int W, std::vector<int64_t> n, bool force, size_t extra) {
    return argo_plan(argo_scratch_size(batch_sized, H, W) + extra, (int)n.size(), offsets(n).data(), H, W, force).records;
  };
  // 800 x 800, 4 x 100,000: 98 regions a frame, 392 in all; SR = min(8, 4096 / 800 = 5) = 5, 160 strips;
  // 392 * 1024 * (8 + 2) = 4,014,080 + 392 * 160 * 4 = 250,880 = 4,264,960 B <= the second half,
  // 256 + 4 * 640,000 * 12 = 30,720,256 B: records.
  EXPECT(path(4, 800, 800, {100000, 100000, 100000, 100000}, false, 0), "known: argo 800 x 800");
  EXPECT(!path(4, 800, 800, {100000, 100000, 100000, 100000}, true, 0), "known: argo forced atomic");
  // 1,100,000 points are 1075 regions > 1024: atomic.
  EXPECT(!path(4, 800, 800, {1100000}, false, 0), "known: argo frame above 1 Mi points");
  // 1 x 1: each half is 256 + 256 = 512 B; one region needs 8,192 B of {z, i} alone: atomic; no points: nothing
  // to place, records; a scratch of 512 + 1 MiB has a second half of 524,544 B >= 8,192 + 2,048 + 4: records.
  EXPECT(!path(1, 1, 1, {1024}, false, 0) && path(1, 1, 1, {0}, false, 0) && path(1, 1, 1, {1024}, false, 1 << 20), "known: argo 1 x 1");
  // 2048 x 2048: SR = 4096 / 2048 = 2, 1024 strips, the most a bin block scans
  const ArgoPlan p = argo_plan(argo_scratch_size(1, 2048, 2048), 1, offsets({5000}).data(), 2048, 2048, false);
  EXPECT(p.strip_rows == 2 && p.strips == 1024 && p.records, "known: argo 2048 x 2048");
  EXPECT(argo_scratch_size(0, 8, 8) == 0 && argo_scratch_size(65, 8, 8) == 0 && argo_scratch_size(1, 2049, 8) == 0 &&
             argo_scratch_size(1, 8, 0) == 0 && argo_scratch_size(2, 800, 800) == 2 * (256 + 2 * 640000 * 12),
         "argo scratch size");
}

int main() {
  const int64_t counts[] = {0, 1, 1023, 1024, 1025, 132880, 277000, 400000, 600000, 1048576, 1200000};
  const int NC = sizeof(counts) / sizeof(counts[0]);
  long plans = 0;
  for (int cap = 1; cap <= SFA_BEV_MAX_BATCH; ++cap) {
    const BevPlan ref = bev_plan(bev_scratch_size(cap), 1, offsets({0}).data(), 0);  // the capacity's own layout
    for (int batch = 1; batch <= cap; ++batch)
      for (int pat = 0; pat < 2 * NC + 1; ++pat) {
        std::vector<int64_t> n(batch);
        for (int b = 0; b < batch; ++b) n[b] = counts[pat < NC ? pat : (b * 3 + pat) % NC];  // uniform, then mixed
        if (pat == 2 * NC) {  // the three-frame batch [~130 k, 1.2 M, ~130 k]
          if (cap < 3 || batch != 3) continue;
          n = {132880, 1200000, 132880};
        }
        const std::vector<int64_t> off = offsets(n, 7);
        for (int flags = 0; flags < 32; ++flags, ++plans) check_kitti(cap, n, off.data(), ref, flags, (pat & 1) ? 4096 + 40 : 0);
      }
  }
  kitti_known_answers();

  const int shapes[][2] = {{800, 800}, {1, 1}, {2048, 2048}, {5, 2048}, {1, 800}, {1, 2048}, {608, 608}, {2048, 1}, {9, 455}};
  for (auto& s : shapes)
    for (int sized : {1, 2, 8, 64})
      for (int batch = 1; batch <= sized; batch += batch < 4 ? 1 : 15)
        for (int pat = 0; pat < 2 * NC; ++pat)
          for (int force = 0; force < 2; ++force)
            for (size_t extra : {(size_t)0, (size_t)12345, (size_t)1 << 22}) {
              std::vector<int64_t> n(batch);
              for (int b = 0; b < batch; ++b) n[b] = counts[pat < NC ? pat : (b * 3 + pat) % NC];
              check_argo(sized, s[0], s[1], n, force != 0, extra);
              ++plans;
            }
  argo_known_answers();
  std::printf("%ld plans, %d bad\n", plans, bad);
  return bad != 0;
}
