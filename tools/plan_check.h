// What the host checks of the gradient plans share (neck_plan_check.cpp, block_plan_check.cpp,
// stem_grad_plan_check.cpp): the failure counter and the two walkers over csrc/grad_plan.h.  Plain C++, included by
// stand-alone programs that each have their own main.
#pragma once

#include <cstdio>
#include <vector>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/grad_plan.h"

static long bad = 0, plans = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      if (bad++ < 20) {              \
        std::printf("BAD: " __VA_ARGS__); \
        std::printf("\n");           \
      }                              \
    }                                \
  } while (0)

// runs of `per` over n items (tiles: grad_tile_at, else grad_chunk_at): every item once, in order, none empty, only
// the last short
static void check_runs(int n, int per, int count, bool tiles, const char* what) {
  std::vector<int> seen((size_t)n, 0);
  int next = 0;
  for (int c = 0; c < count; ++c) {
    const sfa::GradRange r = tiles ? sfa::grad_tile_at(c, n) : sfa::grad_chunk_at(c, n, per);
    EXPECT(r.first == next && r.count >= 1 && r.count <= per && r.first + r.count <= n, "%s: run %d is [%d, +%d) of %d", what,
           c, r.first, r.count, n);
    EXPECT(c == count - 1 || r.count == per, "%s: run %d of %d is short and not the last", what, c, count);
    if (r.first < 0 || r.count < 0 || r.first + r.count > n) return;
    for (int i = 0; i < r.count; ++i) seen[(size_t)r.first + i]++;
    next = r.first + r.count;
  }
  for (int v : seen) EXPECT(v == 1, "%s: an item is covered %d times (n %d per %d)", what, v, n, per);
}

// n workspace regions of len[i] bytes at off[i]: the first at 0, each aligned and ending before the next starts (so
// no two overlap), the last inside `total`
static void check_regions(const size_t* off, const size_t* len, int n, size_t total, const char* what) {
  EXPECT(off[0] == 0, "%s: first region not at 0", what);
  for (int i = 0; i < n; ++i) {
    EXPECT(off[i] % sfa::kGradAlign == 0, "%s: region %d misaligned", what, i);
    EXPECT(off[i] + len[i] <= (i + 1 < n ? off[i + 1] : total), "%s: region %d overlaps the next / the end", what, i);
  }
}
