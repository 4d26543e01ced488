// Stand-alone check of the convolution launchers' host arithmetic (csrc/conv_args.h, csrc/conv_plan.h),
// host only: the multiply-high division, make_seg, every launch check (what a check lets through is
// inside the limits the kernels assume; a refusal carries the status of its cause, restated below from
// the launchers as they were before conv_plan.h), the patch stem's frame chunks, and the dispatch
// predicates of conv.hip on the KFPN model's conv list.  Build with a sanitizer:
//   g++ -std=c++17 -O2 -g -fsanitize=address,undefined tools/conv_plan_check.cpp -o /tmp/conv_plan_check
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <thread>
#include <vector>

#include "../lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc/conv_plan.h"

namespace sfa {
static char g_err[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
}  // namespace sfa
using namespace sfa;

static long long g_checks = 0, g_bad = 0;
#define EXPECT(cond, ...)                \
  do {                                   \
    ++g_checks;                          \
    if (!(cond)) {                       \
      if (++g_bad <= 20) {               \
        std::printf("BAD %s: ", #cond);  \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

// a check's call with the error text cleared first, so a message shows only that call's refusal
#define FRESH(call) (g_err[0] = 0, (call))

static const unsigned long long LIM31 = 1ull << 31;
static float g_mem[4];  // what the dummy pointers point at (never read)
static const float* const P = g_mem;

// ---------------------------------------------------------------- make_fast_div
static inline unsigned fdiv(unsigned n, FastDiv f) {
  return (unsigned)(((unsigned)(((unsigned long long)n * f.m) >> 32) + n) >> f.s);
}
// Quotients wrong among n = k d - 1, k d, k d + 1 for k in [k0, k1) (n <= 2^31 - 1), branch-free.
static unsigned long long fast_div_multiples(unsigned d, FastDiv f, unsigned long long k0, unsigned long long k1) {
  unsigned long long bad = 0;
  const unsigned up = d == 1 ? 1u : 0u;  // (k d + 1) / d = k + 1 only for d = 1
  for (unsigned long long k = k0; k < k1; ++k) {
    const unsigned n = (unsigned)(k * d);
    const unsigned n1 = n + 1 < (unsigned)LIM31 ? n + 1 : n;  // 2^31 itself is outside the range
    bad += (fdiv(n - 1, f) != (unsigned)k - 1) | (fdiv(n, f) != (unsigned)k) | (fdiv(n1, f) != (unsigned)k + (n1 != n ? up : 0u));
  }
  return bad;
}
// d = 1 .. 1024 holds every extent of the model's maps (H / 2 .. H / 32 of inputs of 32 .. 2048). 16 G
// multiples in all, so the (d, range of k) items are shared out among the machine's threads.
static void check_fast_div() {
  constexpr int kParts = 16;
  std::atomic<int> next{0};
  std::atomic<unsigned long long> bad{0}, done{0};
  auto work = [&] {
    for (int item; (item = next.fetch_add(1)) < 1024 * kParts;) {
      const unsigned d = 1 + item / kParts, part = item % kParts;
      const FastDiv f = make_fast_div(d);
      const unsigned long long K = (LIM31 - 1) / d + 1;  // k = 1 .. K - 1
      unsigned long long b = fast_div_multiples(d, f, 1 + (K - 1) * part / kParts, 1 + (K - 1) * (part + 1) / kParts);
      if (part == 0) {
        for (unsigned n = 0; n <= (1u << 20); ++n) b += fdiv(n, f) != n / d;
        b += fdiv((unsigned)(LIM31 - 1), f) != (unsigned)(LIM31 - 1) / d;
      }
      bad += b;
      ++done;
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (std::thread& t : pool) t.join();
  EXPECT(done == 1024ull * kParts && bad == 0, "fast_div: %llu wrong quotients", (unsigned long long)bad);
}

// ---------------------------------------------------------------- make_seg
static void check_make_seg() {
  ConvSeg g;
  for (int k = 1; k <= 7; ++k) {
    make_seg(g, P, 1, 8, 8, 4, k, 1, 0);
    for (int tap = 0; tap < 64; ++tap)
      EXPECT(((tap * g.kdiv_mul) >> g.kdiv_sh) == tap / k, "kdiv k=%d tap=%d", k, tap);
    EXPECT(g.taps == k * k && g.KH == k && g.KW == k, "taps k=%d", k);
  }
  for (int C = 4; C <= 512; ++C) {
    make_seg(g, P, 1, 1, 1, C, 1, 1, 0);
    EXPECT((1 << g.logC) >= C && (g.logC == 0 || (1 << (g.logC - 1)) < C), "logC C=%d", C);
    EXPECT(((C & (C - 1)) != 0) || (1 << g.logC) == C, "logC exact C=%d", C);
  }
  // B H W C 4 around 2^31: 2^31 / (4 C) elements per frame row set
  for (int C : {4, 64, 512})
    for (int B : {1, 3, 16, 64})
      for (int W : {32, 608, 2048, 16384})
        for (long long d = -2; d <= 2; ++d) {
          const long long H = (long long)(LIM31 / (4ull * C * B * W)) + d;
          if (H < 1 || H > 0x7fffffff) continue;
          const unsigned long long bytes = 4ull * B * H * W * C;
          EXPECT(make_seg(g, P, B, (int)H, W, C, 3, 1, 1) == (bytes < LIM31), "make_seg B=%d H=%lld W=%d C=%d", B, H, W, C);
        }
}

// ---------------------------------------------------------------- the launch checks
static ConvArgs base_conv(int B, int H, int W, int C, int k, int stride, int N) {
  ConvArgs a;
  std::memset(&a, 0, sizeof a);
  a.nseg = 1;
  make_seg(a.seg[0], P, B, H, W, C, k, stride, k / 2);
  a.Kpad = (int)align_up((size_t)k * k * C, 16);
  a.OH = H / stride;
  a.OW = W / stride;
  a.M = B * a.OH * a.OW;
  a.N = N;
  a.w = a.winv = a.bias = P;
  a.wx = a.wh = reinterpret_cast<const uint16_t*>(g_mem);
  a.y = g_mem;
  a.relu = 1;
  return a;
}

// The status each launcher returned at the parent commit, restated cause by cause in its order.
static bool aligned(const ConvArgs& a, int BK, int BN) {
  return !(a.Kpad % BK != 0 || (a.nseg == 2 && a.kseg1 % BK != 0) || a.N % BN != 0);
}
static bool grid_ok(const ConvArgs& a, int BM, int BN, int ks, long long* n) {
  *n = ((long long)a.M + BM - 1) / BM * (a.N / BN) * ks;
  return *n > 0 && *n <= 0x7fffffffll;
}
static bool splitk_bad(const ConvArgs& a, int epi, int units) {
  const int ks = a.ksplit > 1 ? a.ksplit : 1;
  return ks > 1 && (epi != EPI_STD || units % ks != 0 || !a.part || (size_t)ks * a.M * a.N > a.part_floats || a.N % 4 != 0);
}
static bool slice_bad(const ConvArgs& a) { return a.wstride && (a.wstride < a.wk0 + a.Kpad || a.wk0 % 8 != 0); }
static unsigned long long wbytes(const ConvArgs& a, int terms, bool strided) {
  return (unsigned long long)terms * a.N * (strided && a.wstride ? a.wstride : a.Kpad) * 2ull;
}

static int old_h3(const ConvArgs& a, int BM, int BN, int BK, int epi, int terms) {
  long long n;
  if (!a.wh || !a.winv || !aligned(a, BK, BN)) return SFA_E_UNSUPPORTED;
  if (slice_bad(a)) return SFA_E_INVALID;
  if (wbytes(a, 2, true) >= LIM31) return SFA_E_UNSUPPORTED;
  if (splitk_bad(a, epi, a.Kpad / BK)) return SFA_E_UNSUPPORTED;
  if (!grid_ok(a, BM, BN, a.ksplit > 1 ? a.ksplit : 1, &n)) return SFA_E_INVALID;
  if (a.res_up && (a.nseg != 1 || terms != 2)) return SFA_E_UNSUPPORTED;
  return SFA_OK;
}
static int old_h3s(const ConvArgs& a, int BM, int BN, int epi) {
  const ConvSeg& g = a.seg[0];
  long long n;
  if (!a.wh || !a.winv || a.nseg != 1 || g.KH != 3 || g.KW != 3 || g.stride != 1 || g.pad != 1 || g.C < 32 ||
      (g.C & 31) != 0 || a.Kpad != 9 * g.C || a.OH != g.H || a.OW != g.W || a.N % BN != 0)
    return SFA_E_UNSUPPORTED;
  if (a.wstride || a.wk0 || a.res_up) return SFA_E_UNSUPPORTED;  // the hardening: the parent let these through
  if (a.OH * a.OW < (BM > 128 ? BM : 128)) return SFA_E_UNSUPPORTED;
  if (splitk_bad(a, epi, 3 * (g.C >> 5))) return SFA_E_UNSUPPORTED;
  if (wbytes(a, 2, false) >= LIM31) return SFA_E_UNSUPPORTED;
  return grid_ok(a, BM, BN, a.ksplit > 1 ? a.ksplit : 1, &n) ? SFA_OK : SFA_E_INVALID;
}
static int old_r3(const ConvArgs& a, int BM, int BN, int epi, bool ru, bool st, bool cm) {
  long long n;
  if (!a.wh || !a.winv || !aligned(a, 32, BN) || (a.res_up && (!ru || a.res || a.nseg != 1))) return SFA_E_UNSUPPORTED;
  if (st && (a.nseg != 1 || a.seg[0].C < 32 || a.seg[0].taps > 32)) return SFA_E_UNSUPPORTED;
  if (cm && (a.seg[0].taps != 9 || a.seg[0].C % 32 != 0 || (a.nseg == 2 ? a.kseg1 : a.Kpad) != 9 * a.seg[0].C ||
             a.Kpad / 32 > 3600 || a.wstride || a.wk0))
    return SFA_E_UNSUPPORTED;
  for (int s = 0; s < a.nseg; ++s)
    if (a.seg[s].C < 8) return SFA_E_UNSUPPORTED;
  if (slice_bad(a)) return SFA_E_INVALID;
  if (wbytes(a, 2, true) >= LIM31) return SFA_E_UNSUPPORTED;
  if (splitk_bad(a, epi, a.Kpad / 32)) return SFA_E_UNSUPPORTED;
  return grid_ok(a, BM, BN, a.ksplit > 1 ? a.ksplit : 1, &n) ? SFA_OK : SFA_E_INVALID;
}
static int old_x6(const ConvArgs& a, bool have_w, int BM, int BN, int BK) {
  long long n;
  if (!have_w || !aligned(a, BK, BN)) return SFA_E_UNSUPPORTED;
  if (wbytes(a, 3, false) >= LIM31) return SFA_E_UNSUPPORTED;
  return grid_ok(a, BM, BN, 1, &n) ? SFA_OK : SFA_E_INVALID;
}
static int old_f32(const ConvArgs& a, int BM, int BN, int BK) {
  long long n;
  if (!aligned(a, BK, BN)) return SFA_E_UNSUPPORTED;
  return grid_ok(a, BM, BN, 1, &n) ? SFA_OK : SFA_E_INVALID;
}

// What every accepted launch must satisfy, whatever family let it through.
static void accepted(const char* fam, const ConvArgs& a, unsigned grid, int terms, bool strided, int BM) {
  const int ks = std::strcmp(fam, "x6") && a.ksplit > 1 ? a.ksplit : 1;  // conv_x6 / x6g never split
  EXPECT(grid >= 1 && grid <= 0x7fffffffu, "%s grid %u", fam, grid);
  EXPECT(ks == 1 || (a.part && (unsigned long long)ks * a.M * a.N <= a.part_floats), "%s split-K partials ks=%d", fam, ks);
  EXPECT(wbytes(a, terms, strided) < LIM31, "%s term bytes N=%d Kpad=%d wstride=%d", fam, a.N, a.Kpad, a.wstride);
  EXPECT(!strided || !a.wstride || (a.wk0 >= 0 && a.wk0 + a.Kpad <= a.wstride), "%s slice wk0=%d Kpad=%d wstride=%d", fam,
         a.wk0, a.Kpad, a.wstride);
  if (!std::strcmp(fam, "h3s")) {
    EXPECT(a.OH * a.OW >= 128 && a.OH * a.OW >= BM, "h3s frames of %d rows", a.OH * a.OW);
    EXPECT(!a.wstride && !a.wk0 && !a.res_up, "h3s sliced");
  }
}

static void run_families(const ConvArgs& a) {
  unsigned grid = 0;
  struct Tile { int BM, BN, BK; };
  for (Tile t : {Tile{128, 64, 32}, Tile{128, 128, 32}, Tile{64, 128, 16}, Tile{256, 64, 32}, Tile{256, 320, 32}}) {
    for (int epi : {(int)EPI_STD, (int)EPI_HEAD})
      for (int terms : {1, 2}) {
        int rc = FRESH(conv_h3_check(a, t.BM, t.BN, t.BK, epi, terms, &grid));
        EXPECT(rc == old_h3(a, t.BM, t.BN, t.BK, epi, terms), "h3 rc %d (%s)", rc, g_err);
        if (rc == SFA_OK) accepted("h3", a, grid, 2, true, t.BM);
      }
    for (int epi : {(int)EPI_STD, (int)EPI_HEAD}) {
      int rc = FRESH(conv_h3s_check(a, t.BM, t.BN, epi, &grid));
      EXPECT(rc == old_h3s(a, t.BM, t.BN, epi), "h3s rc %d (%s)", rc, g_err);
      if (rc == SFA_OK) accepted("h3s", a, grid, 2, false, t.BM);
      for (int opt = 0; opt < 8; ++opt) {
        const bool ru = opt & 1, st = opt & 2, cm = opt & 4;
        rc = FRESH(conv_r3_check(a, t.BM, t.BN, epi, ru, st, cm, &grid));
        EXPECT(rc == old_r3(a, t.BM, t.BN, epi, ru, st, cm), "r3 rc %d opt %d (%s)", rc, opt, g_err);
        if (rc == SFA_OK) accepted("r3", a, grid, 2, true, t.BM);
      }
    }
    for (bool have_w : {false, true}) {
      int rc = FRESH(conv_x6_check("conv_x6", a, have_w, t.BM, t.BN, t.BK, &grid));
      EXPECT(rc == old_x6(a, have_w, t.BM, t.BN, t.BK), "x6 rc %d (%s)", rc, g_err);
      if (rc == SFA_OK) accepted("x6", a, grid, 3, false, t.BM);
      rc = FRESH(conv_x6_check("conv_x6g", a, have_w, t.BM, t.BN, 16, &grid));
      EXPECT(rc == old_x6(a, have_w, t.BM, t.BN, 16), "x6g rc %d (%s)", rc, g_err);
      if (rc == SFA_OK) accepted("x6", a, grid, 3, false, t.BM);
    }
    int rc = FRESH(conv_f32_check(a, t.BM, t.BN, t.BK, &grid));
    EXPECT(rc == old_f32(a, t.BM, t.BN, t.BK), "f32 rc %d (%s)", rc, g_err);
    if (rc == SFA_OK) EXPECT(grid >= 1 && grid <= 0x7fffffffu, "f32 grid %u", grid);
  }
}

static std::vector<int> around(std::initializer_list<long long> vs) {
  std::vector<int> r;
  for (long long v : vs)
    for (long long d = -1; d <= 1; ++d)
      if (v + d >= -1 && v + d <= 0x7fffffffll) r.push_back((int)(v + d));
  return r;
}

static void check_families() {
  const ConvArgs b0 = base_conv(2, 24, 24, 64, 3, 1, 128);  // a strip-shaped 3x3 conv, Kpad 576
  run_families(b0);
  // M: empty, one row, the tile heights, the grid bound (M / BM * N / BN * ks around 2^31)
  for (int M : around({0, 1, 64, 128, 256, 1 << 20, 0x7fffffffll}))
    for (int N : {64, 128, 320, 512, 1 << 20, 1 << 24}) {
      ConvArgs a = b0;
      a.M = M;
      a.N = N;
      run_families(a);
      a.ksplit = 2;
      a.part = g_mem;
      a.part_floats = ~(size_t)0;
      run_families(a);
    }
  // N and Kpad: tile widths, the K-tile depths, the 2 GiB weight bound for 2 and 3 terms
  for (int N : around({0, 4, 64, 128, 320, 512}))
    for (int K : around({16, 32, 288, 576, 3600 * 32, (long long)(LIM31 / (4ull * 128)), (long long)(LIM31 / (6ull * 128))})) {
      ConvArgs a = b0;
      a.N = N;
      a.Kpad = K;
      run_families(a);
    }
  for (int N : {128, 512})
    for (long long K : {(long long)(LIM31 / (4ull * N)), (long long)(LIM31 / (6ull * N))})
      for (long long d = -32; d <= 32; d += 16) {
        ConvArgs a = b0;
        a.N = N;
        a.Kpad = (int)(K + d);
        run_families(a);
        a.wstride = a.Kpad;  // the same bound through the row stride
        a.Kpad = 576;
        run_families(a);
      }
  // two segments: kseg1 around the K-tile depths and the chunk-major first segment
  for (int nseg : {1, 2})
    for (int kseg1 : around({0, 16, 32, 576, 592})) {
      ConvArgs a = b0;
      a.nseg = nseg;
      a.kseg1 = kseg1;
      a.Kpad = 576 + 64;
      make_seg(a.seg[1], P, 2, 48, 48, 64, 1, 2, 0);
      run_families(a);
    }
  // split-K: slice counts against the K units, the partial buffer's capacity around ks M N
  for (int ks : {-1, 0, 1, 2, 3, 4, 6, 18, 19})
    for (int sz : {-1, 0, 1})
      for (int with_part : {0, 1}) {
        ConvArgs a = b0;
        a.ksplit = ks;
        a.part = with_part ? g_mem : nullptr;
        a.part_floats = (size_t)((long long)(ks > 1 ? ks : 1) * a.M * a.N + sz);
        run_families(a);
      }
  // K slices: stride and first column around the slice's end, unaligned starts
  for (int wstride : around({0, 576, 1152}))
    for (int wk0 : around({0, 4, 8, 12, 576, 580})) {  // 4, 12, 580: multiples of 4 that are none of 8
      if (wstride < 0 || wk0 < 0) continue;
      ConvArgs a = b0;
      a.wstride = wstride;
      a.wk0 = wk0;
      run_families(a);
      a.res_up = P;
      run_families(a);
      a.res = P;
      run_families(a);
    }
  // frame rows around the strip kernel's 128 and 256 (h3s), with batches that keep M large
  for (int rows : around({128, 256}))
    for (int B : {1, 16}) {
      ConvArgs a = base_conv(B, 1, rows, 64, 3, 1, 128);
      run_families(a);
    }
  for (int hw : {3, 6, 11, 12, 16}) run_families(base_conv(4, hw, hw, 256, 3, 1, 256));
  // missing weights
  {
    ConvArgs a = b0;
    a.wh = nullptr;
    run_families(a);
    a = b0;
    a.winv = nullptr;
    run_families(a);
  }
  // narrow / odd channel counts (conv_r3's 8-channel rule, the strip's 32-channel chunks)
  for (int C : {4, 8, 16, 32, 64}) run_families(base_conv(2, 24, 24, C, 3, 1, 128));
  for (int k : {1, 3, 7}) run_families(base_conv(2, 24, 24, 64, k, 1, 128));

  // launch_conv's shape checks
  {
    ConvArgs a = b0;
    EXPECT(FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_FP16X3)) == SFA_OK, "shape base (%s)", g_err);
    for (int N : around({0, 64, 128})) {
      a = b0;
      a.N = N;
      EXPECT(FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_F32)) == (N > 0 && N % 64 == 0 ? SFA_OK : SFA_E_UNSUPPORTED), "shape N=%d", N);
    }
    for (int K : around({0, 16, 576})) {
      a = b0;
      a.Kpad = K;
      EXPECT(FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_F32)) == (K > 0 && K % 16 == 0 ? SFA_OK : SFA_E_UNSUPPORTED), "shape K=%d", K);
    }
    for (int M : {-1, 0, 1}) {
      a = b0;
      a.M = M;
      EXPECT(FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_F32)) == (M > 0 ? SFA_OK : SFA_E_UNSUPPORTED), "shape M=%d", M);
    }
    for (int C : {2, 4, 8, 12, 16, 48, 64}) {
      a = b0;
      a.seg[0].C = C;
      a.seg[0].logC = ilog2(C);
      EXPECT(FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_F32)) == (C >= 4 && !(C & (C - 1)) ? SFA_OK : SFA_E_UNSUPPORTED), "shape C=%d", C);
    }
    for (unsigned long long by : {0ull, 1ull, LIM31 - 1, LIM31, LIM31 + 1}) {
      a = b0;
      a.seg[0].bytes = (unsigned)by;
      EXPECT(FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_F32)) == (by > 0 && by < LIM31 ? SFA_OK : SFA_E_UNSUPPORTED), "shape bytes=%llu", by);
    }
    for (int kseg1 : around({0, 16, 576, 640})) {
      a = b0;
      a.nseg = 2;
      a.seg[1] = a.seg[0];
      a.Kpad = 640;
      a.kseg1 = kseg1;
      EXPECT(FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_F32)) == (kseg1 > 0 && kseg1 < 640 && kseg1 % 16 == 0 ? SFA_OK : SFA_E_UNSUPPORTED),
             "shape kseg1=%d", kseg1);
    }
    a = b0;
    a.nseg = 2;
    a.kseg1 = 16;
    a.seg[1] = a.seg[0];
    a.seg[0].C = 4;
    a.seg[0].logC = 2;  // a narrow segment ahead of a wide one
    EXPECT(FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_F32)) == SFA_E_UNSUPPORTED, "narrow first");
    for (int math : {(int)SFA_MATH_F32, (int)SFA_MATH_BF16X6, (int)SFA_MATH_FP16X3, (int)SFA_MATH_FP16})
      for (int epi : {(int)EPI_STD, (int)EPI_HEAD})
        for (int odd : {0, 1})
          for (int res : {0, 1}) {
            a = b0;
            a.res_up = P;
            a.OH += odd;
            a.res = res ? P : nullptr;
            const bool ok = math == SFA_MATH_FP16X3 && epi == EPI_STD && !odd && !res;
            EXPECT(FRESH(conv_shape_check(a, epi, math)) == (ok ? SFA_OK : SFA_E_UNSUPPORTED), "shape res_up math=%d epi=%d", math, epi);
          }
  }

  // deconv: 128 x 128 tiles, four phases
  for (int B : {0, 1, 16})
    for (int H : {0, 1, 19, 16383, 16384})
      for (int C : {16, 32, 48, 512})
        for (int N : around({0, 128, 256})) {
          DeconvArgs d;
          std::memset(&d, 0, sizeof d);
          d.x = d.winv = d.bias = P;
          d.wh = reinterpret_cast<const uint16_t*>(g_mem);
          d.y = g_mem;
          d.H = H;
          d.W = 19;
          d.C = C;
          d.logC = ilog2(C);
          d.N = N;
          d.K = 4 * C;
          const unsigned long long in_bytes = 4ull * B * H * 19 * C;
          d.bytes = (unsigned)in_bytes;
          d.M = B * H * 19;
          unsigned grid = 0;
          const int rc = FRESH(deconv_check(d, B, 128, 128, &grid));
          const int want = B < 1 || H < 1 ? SFA_E_INVALID
                           : (C < 32 || (C & (C - 1)) || N <= 0 || N % 128) ? SFA_E_UNSUPPORTED
                           : (in_bytes >= LIM31 || H >= 16384) ? SFA_E_UNSUPPORTED
                                                                : SFA_OK;
          EXPECT(rc == want, "deconv B=%d H=%d C=%d N=%d rc %d (%s)", B, H, C, N, rc, g_err);
          if (rc == SFA_OK)
            EXPECT(grid == 4u * ((d.M + 127) / 128) * (N / 128) && 8ull * N * d.K < LIM31 * 2, "deconv grid %u", grid);
        }

  // the patch stem: 16 x 16 conv-output tiles, the side buffer's 17 rows of 64 floats per tile
  for (int H : {32, 64, 96, 608, 624})
    for (int with_part : {0, 1})
      for (int sz : {-1, 0, 1}) {
        ConvArgs a = base_conv(2, H, 96, 4, 7, 2, 64);
        a.part = with_part ? g_mem : nullptr;
        a.part_floats = (size_t)((long long)a.M / 256 * 17 * 64 + sz);
        const bool shape = (H / 2) % 16 == 0;
        const int want = !shape ? SFA_E_UNSUPPORTED : !with_part ? SFA_E_INVALID : sz < 0 ? SFA_E_UNSUPPORTED : SFA_OK;
        const int rc = FRESH(stem_patch_check(a));
        EXPECT(rc == want, "stem H=%d part=%d sz=%d rc %d (%s)", H, with_part, sz, rc, g_err);
      }
}

// ---------------------------------------------------------------- the patch stem's frame chunks
static void check_stem_chunks() {
  // 32 x 32 .. a frame above 2^31 - 1 bytes (3 channels: 13408^2 x 12 B, 4: 11616^2 x 16 B)
  const int sizes[] = {32, 64, 608, 1216, 2048, 4096, 8192, 11584, 11616, 13376, 13408};
  for (int S : sizes)
    for (int ch : {3, 4})
      for (int B = 1; B <= 64; ++B) {
        const unsigned long long fbytes = (unsigned long long)ch * S * S * 4;
        StemChunks p;
        const int rc = FRESH(stem_chunk_plan(B, ch, S, S, &p));
        if (fbytes > LIM31 - 1) {
          EXPECT(rc == SFA_E_UNSUPPORTED, "stem chunks: %d-channel %d^2 frame accepted", ch, S);
          continue;
        }
        EXPECT(rc == SFA_OK, "stem chunks: %d x %d^2 refused (%s)", B, S, g_err);
        if (rc != SFA_OK) continue;
        const size_t tpf = (size_t)(S / 32) * (S / 32);
        int next = 0;
        for (int i = 0; i < p.count(); ++i) {
          const StemChunk c = stem_chunk(p, i, S, S);
          EXPECT(c.f0 == next && c.frames >= 1, "stem chunk %d starts at %d, expected %d", i, c.f0, next);
          EXPECT(c.x_bytes < LIM31 && c.x_bytes == (unsigned long long)c.frames * fbytes, "stem chunk bytes %zu", c.x_bytes);
          EXPECT(c.x_floats == (size_t)c.f0 * (fbytes / 4), "stem chunk input offset");
          EXPECT(c.part_floats == (size_t)c.f0 * tpf * 17 * 64, "stem chunk side-buffer offset");
          EXPECT(c.y_floats == (size_t)c.f0 * (S / 4) * (S / 4) * 64, "stem chunk output offset");
          EXPECT(c.tiles == (long long)c.frames * (long long)tpf, "stem chunk tiles");
          next = c.f0 + c.frames;
        }
        EXPECT(next == B, "stem chunks cover %d of %d frames", next, B);
      }
  StemChunks p;
  EXPECT(FRESH(stem_chunk_plan(16, 3, 608, 608, &p)) == SFA_OK && p.count() == 1, "16 x 608 x 608: one chunk");
  EXPECT(FRESH(stem_chunk_plan(16, 4, 608, 608, &p)) == SFA_OK && p.count() == 1, "16 x 608 x 608 x 4: one chunk");
}

// ---------------------------------------------------------------- the product's conv list
// The KFPN model's launches (model.hip): the 16 launches of layer1..4 (19 convs: the three 1x1 / stride-2
// downsamples ride as second K-segments; the stem is the patch kernel's, above), the FPN's commuted
// 1x1 convs and the three head launches. What conv.hip's rules ask of them at an input of B x H x W.
struct Outcome {
  bool strip, h3s_ok, big, mid;
  int ksplit;
  bool operator==(const Outcome& o) const {
    return strip == o.strip && h3s_ok == o.h3s_ok && big == o.big && mid == o.mid && ksplit == o.ksplit;
  }
};

static std::vector<Outcome> product(int B, int H, int W) {
  std::vector<Outcome> out;
  const size_t part_floats = (size_t)2 * B * (H / 32) * (W / 32) * 512;
  int ih = H / 4, iw = W / 4, ic = 64;
  for (int li = 0; li < 4; ++li) {
    const int planes = 64 << li, stride = li == 0 ? 1 : 2, oh = ih / stride, ow = iw / stride;
    for (int k = 0; k < 4; ++k) {
      ConvArgs a = k == 0 ? base_conv(B, ih, iw, ic, 3, stride, planes) : base_conv(B, oh, ow, planes, 3, 1, planes);
      if (k == 1 && li > 0) {  // + the block's input through the 1x1 / stride-2 downsample
        a.nseg = 2;
        a.kseg1 = 9 * planes;
        a.Kpad = 9 * planes + ic;
        make_seg(a.seg[1], P, B, ih, iw, ic, 1, stride, 0);
      }
      a.part = g_mem;
      a.part_floats = part_floats;
      EXPECT(FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_FP16X3)) == SFA_OK, "layer%d conv %d shape (%s)", li + 1, k, g_err);
      Outcome o;
      o.strip = strip_ok(a);
      o.ksplit = pick_ksplit(a);
      o.big = tile_rows(a) >= 50000;
      o.mid = tile_rows(a) >= 10000;
      EXPECT(o.strip == !(li > 0 && k < 2), "layer%d conv %d strip_ok %d", li + 1, k, o.strip);
      EXPECT(o.ksplit == (li == 3 ? 2 : 1), "layer%d conv %d ksplit %d", li + 1, k, o.ksplit);
      a.ksplit = o.ksplit;
      unsigned grid = 0;
      const int BN = planes == 64 ? 64 : 128;
      o.h3s_ok = o.strip && FRESH(conv_h3s_check(a, 128, BN, EPI_STD, &grid)) == SFA_OK;
      EXPECT(o.h3s_ok == (o.strip && oh * ow >= 128), "layer%d conv %d h3s at %d rows", li + 1, k, oh * ow);
      if (!o.h3s_ok) {  // what the strip kernel refuses, conv_h3 takes (conv_r3 on the big-M side)
        if ((a.Kpad / 32) % a.ksplit != 0) a.ksplit = 1;
        const int rc = planes == 64 ? FRESH(conv_h3_check(a, 256, 64, 32, EPI_STD, 2, &grid))
                                    : FRESH(conv_h3_check(a, 128, 128, 32, EPI_STD, 2, &grid));
        EXPECT(rc == SFA_OK, "layer%d conv %d conv_h3 rc %d (%s)", li + 1, k, rc, g_err);
        if (o.big && planes != 64)
          EXPECT(FRESH(conv_r3_check(a, 128, 128, EPI_STD, false, false, true, &grid)) == SFA_OK, "layer%d conv %d conv_r3 (%s)", li + 1,
                 k, g_err);
      }
      out.push_back(o);
    }
    ih = oh;
    iw = ow;
    ic = planes;
  }
  // FPN level f: W_a . lo at the low resolution (no bias), then W_b . skip + b + up2x of it
  const int loc[3] = {512, 256, 128}, skc[3] = {256, 128, 64}, nout[3] = {256, 128, 64};
  for (int f = 0; f < 3; ++f) {
    const int lh = H >> (5 - f), lw = W >> (5 - f);
    ConvArgs lo = base_conv(B, lh, lw, loc[f], 1, 1, nout[f]);
    lo.bias = nullptr;
    lo.wstride = loc[f] + skc[f];
    lo.part = g_mem;
    lo.part_floats = part_floats;
    ConvArgs sk = base_conv(B, 2 * lh, 2 * lw, skc[f], 1, 1, nout[f]);
    sk.wstride = lo.wstride;
    sk.wk0 = loc[f];
    sk.res_up = P;
    sk.part = g_mem;
    sk.part_floats = part_floats;
    for (const ConvArgs* a : {&lo, &sk}) {
      EXPECT(FRESH(conv_shape_check(*a, EPI_STD, SFA_MATH_FP16X3)) == SFA_OK, "fpn %d shape (%s)", f, g_err);
      EXPECT(pick_ksplit(*a) == 1 && !(strip_ok(*a)), "fpn %d split / strip", f);
      unsigned grid = 0;
      EXPECT(FRESH(conv_h3s_check(*a, 128, 64, EPI_STD, &grid)) == SFA_E_UNSUPPORTED, "fpn %d on the strip kernel", f);
      out.push_back(Outcome{false, false, tile_rows(*a) >= 50000, tile_rows(*a) >= 10000, 1});
    }
    EXPECT(fpn_1x1_ok(lo, loc[f], 64) && !lo.res_up, "fpn %d low-resolution conv on fpn_gemm", f);
    EXPECT(fpn_skip_ok(sk, skc[f], 64), "fpn %d skip conv on fpn_row / fpn_seg", f);
    unsigned grid = 0;
    EXPECT(FRESH(conv_r3_check(sk, 128, nout[f] == 64 ? 64 : 128, EPI_STD, true, false, false, &grid)) == SFA_OK, "fpn %d skip conv on conv_r3 (%s)",
           f, g_err);
    EXPECT(FRESH(conv_h3_check(lo, 64, 128 > nout[f] ? 64 : 128, 32, EPI_STD, 2, &grid)) == SFA_OK, "fpn %d low conv on conv_h3 (%s)", f, g_err);
  }
  // heads of levels 0 / 1 / 2: all five heads of a level, 5 x 64 = 320 columns
  const int hc[3] = {256, 128, 64}, hs[3] = {8, 4, 4};
  for (int f = 0; f < 3; ++f) {
    ConvArgs a = base_conv(B, H / hs[f], W / hs[f], hc[f], 3, 1, 320);
    unsigned grid = 0;
    EXPECT(FRESH(conv_shape_check(a, EPI_HEAD, SFA_MATH_FP16X3)) == SFA_OK, "heads %d shape (%s)", f, g_err);
    const int rc = FRESH(conv_r3_check(a, 256, 320, EPI_HEAD, false, true, true, &grid));
    EXPECT(rc == SFA_OK && grid == (unsigned)((a.M + 255) / 256), "heads %d conv_r3 rc %d (%s)", f, rc, g_err);
    EXPECT(pick_ksplit(a) == 1, "heads %d split", f);
    out.push_back(Outcome{strip_ok(a), false, tile_rows(a) >= 50000, tile_rows(a) >= 10000, 1});
  }
  return out;
}

// Which side of tile_rows >= 50000 (big) and >= 10000 (mid) every launch of product() falls on, from the
// rows of a frame at layer1..4 written out by hand (tile_rows = 16 rows): the four convs of layer l at rows[l],
// FPN level f's low-resolution conv at rows[3 - f] and its skip conv at rows[2 - f], the heads at rows[1],
// rows[0], rows[0].
static void expect_sides(const char* shape, const std::vector<Outcome>& v, const int (&rows)[4], const bool (&big)[4],
                         const bool (&mid)[4]) {
  int level[25];
  for (int i = 0; i < 16; ++i) level[i] = i / 4;
  for (int f = 0; f < 3; ++f) {
    level[16 + 2 * f] = 3 - f;
    level[17 + 2 * f] = 2 - f;
  }
  level[22] = 1;
  level[23] = level[24] = 0;
  EXPECT(v.size() == 25, "%s: %zu launches", shape, v.size());
  for (size_t i = 0; i < v.size() && i < 25; ++i) {
    const int l = level[i];
    EXPECT(big[l] == (16LL * rows[l] >= 50000) && mid[l] == (16LL * rows[l] >= 10000), "%s: table of level %d", shape, l);
    EXPECT(v[i].big == big[l] && v[i].mid == mid[l], "%s: launch %zu (%d rows) big %d mid %d", shape, i, rows[l], v[i].big,
           v[i].mid);
  }
}

static void check_product() {
  const std::vector<Outcome> a1 = product(1, 608, 608), a16 = product(16, 608, 608);
  EXPECT(a1 == a16, "608 x 608: an outcome depends on the batch");
  for (int li = 0; li < 4; ++li)
    for (int k = 0; k < 4; ++k) {
      const Outcome& o = a16[4 * li + k];
      // layer1 / layer2 (152^2, 76^2 rows) on the big-M side, layer3 (38^2) between the bounds, layer4 (19^2) below both
      EXPECT(o.big == (li < 2) && o.mid == (li < 3), "608: layer%d conv %d tile_rows side", li + 1, k);
      EXPECT(o.ksplit == (li == 3 ? 2 : 1), "608: layer%d conv %d ksplit", li + 1, k);
      EXPECT(o.h3s_ok == o.strip, "608: layer%d conv %d strip kernel", li + 1, k);
    }
  EXPECT(a16[4].big && a16[5].big && !a16[4].strip && !a16[5].strip, "608: layer2's stride-2 convs take conv_r3");
  EXPECT(!a16[8].big && !a16[9].big, "608: layer3's stride-2 convs stay on conv_h3");
  const std::vector<Outcome> s384 = product(1, 384, 384), s352 = product(1, 352, 352);
  EXPECT(s384[14].strip && s384[14].h3s_ok && s384[14].ksplit == 2, "384: layer4 (144 rows) on the strip kernel, split by 2");
  EXPECT(s352[14].strip && !s352[14].h3s_ok, "352: layer4 (121 rows) refused by the strip kernel");
  const std::vector<Outcome> s96 = product(2, 96, 96), s64 = product(4, 64, 96);
  EXPECT(s96[2].h3s_ok && s96[6].h3s_ok && !s96[10].h3s_ok && !s96[14].h3s_ok, "2 x 96 x 96: layer3 / 4 maps refused by h3s");
  EXPECT(s64[2].h3s_ok && !s64[6].h3s_ok && !s64[10].h3s_ok && !s64[14].h3s_ok, "4 x 64 x 96: layer2..4 maps refused by h3s");
  for (const auto* v : {&s384, &s96, &s64})
    for (size_t i = 0; i < 16; ++i) EXPECT((*v)[i].ksplit == (i >= 12 ? 2 : 1), "ksplit of conv %zu", i);
  expect_sides("608", a16, {152 * 152, 76 * 76, 38 * 38, 19 * 19}, {true, true, false, false}, {true, true, true, false});
  expect_sides("608 B=1", a1, {152 * 152, 76 * 76, 38 * 38, 19 * 19}, {true, true, false, false}, {true, true, true, false});
  expect_sides("384", s384, {96 * 96, 48 * 48, 24 * 24, 12 * 12}, {true, false, false, false}, {true, true, false, false});
  expect_sides("96", s96, {24 * 24, 12 * 12, 6 * 6, 3 * 3}, {false, false, false, false}, {false, false, false, false});
  expect_sides("64x96", s64, {16 * 24, 8 * 12, 4 * 6, 2 * 3}, {false, false, false, false}, {false, false, false, false});
  EXPECT(product(1, 96, 96) == product(2, 96, 96) && product(1, 64, 96) == s64, "small maps: an outcome depends on the batch");
}

// ---------------------------------------------------------------- the body convs' rule table
// conv_plan.h body_conv_rule on the sixteen residual-layer launches, layer li + 1 (li = 0..3), conv k = 2 block +
// conv: as model.hip builds them for a B x H x W input, and as block.hip builds the two of one block for a caller's
// B x h x w map (odd sizes round up at stride 2; the partial buffer only where the block is 512 wide).
static ConvArgs model_body_conv(int B, int H, int W, int li, int k) {
  const int planes = 64 << li, stride = li == 0 ? 1 : 2, ic = li == 0 ? 64 : planes / 2;
  const int ih = (H / 4) >> (li > 0 ? li - 1 : 0), iw = (W / 4) >> (li > 0 ? li - 1 : 0), oh = ih / stride, ow = iw / stride;
  ConvArgs a = k == 0 ? base_conv(B, ih, iw, ic, 3, stride, planes) : base_conv(B, oh, ow, planes, 3, 1, planes);
  if (k == 1 && li > 0) {
    a.nseg = 2;
    a.kseg1 = 9 * planes;
    a.Kpad = 9 * planes + ic;
    make_seg(a.seg[1], P, B, ih, iw, ic, 1, stride, 0);
  }
  a.part = g_mem;
  a.part_floats = (size_t)2 * B * (H / 32) * (W / 32) * 512;
  return a;
}

static ConvArgs block_body_conv(int B, int h, int w, int li, int block, int c) {
  const int planes = 64 << li, ds = block == 0 && li > 0, stride = ds ? 2 : 1, ic = ds ? planes / 2 : planes;
  const int oh = (h + stride - 1) / stride, ow = (w + stride - 1) / stride;
  ConvArgs a = c == 0 ? base_conv(B, h, w, ic, 3, stride, planes) : base_conv(B, oh, ow, planes, 3, 1, planes);
  a.OH = oh;
  a.OW = ow;
  a.M = B * oh * ow;
  if (c == 1 && ds) {
    a.nseg = 2;
    a.kseg1 = 9 * planes;
    a.Kpad = 9 * planes + ic;
    make_seg(a.seg[1], P, B, h, w, ic, 1, stride, 0);
  }
  if (planes >= 512) {
    a.part = g_mem;
    a.part_floats = (size_t)2 * a.M * planes;
  }
  return a;
}

// The tile and the slices each rule stands for, written out again: what strip_tile_bn and the launch must agree with.
struct RuleTile { int fam, BM, BN, ks; };  // fam: 0 none, 1 conv_h3s, 2 conv_r3 (R3_BODY), 3 conv_h3
static RuleTile rule_tile(BodyRule r) {
  switch (r) {
    case BODY_STRIP_128x64: return {1, 128, 64, 1};
    case BODY_STRIP_64x128: return {1, 64, 128, 1};
    case BODY_STRIP_128x64_KS2: return {1, 128, 64, 2};
    case BODY_STRIP_128x128: return {1, 128, 128, 1};
    case BODY_STRIP_128x128_KS2: return {1, 128, 128, 2};
    case BODY_R3: return {2, 128, 128, 1};
    case BODY_R3_KS2: return {2, 128, 128, 2};
    case BODY_H3_256x64: return {3, 256, 64, 1};
    case BODY_H3_128x64: return {3, 128, 64, 1};
    case BODY_H3_128x128: return {3, 128, 128, 1};
    case BODY_H3_128x128_KS2: return {3, 128, 128, 2};
    default: return {0, 0, 0, 1};
  }
}

// The chosen instance's own check on the launch as launch_conv_h makes it (ksplit from the rule).
static int rule_check(const ConvArgs& a, BodyRule r, unsigned* grid) {
  const RuleTile t = rule_tile(r);
  ConvArgs b = a;
  b.ksplit = t.ks;
  if (t.fam == 1) return FRESH(conv_h3s_check(b, t.BM, t.BN, EPI_STD, grid));
  if (t.fam == 2) return FRESH(conv_r3_check(b, t.BM, t.BN, EPI_STD, false, false, true, grid));
  if (t.fam == 3) return FRESH(conv_h3_check(b, t.BM, t.BN, r == BODY_H3_128x64 ? 16 : 32, EPI_STD, 2, grid));
  return SFA_E_UNSUPPORTED;
}

static const int kWalkMax = 2048;
static long long g_first[BODY_RULE_COUNT][3];  // the smallest input (pixels, H, W) that reaches each rule

static void check_body_rules() {
  for (int r = 0; r < BODY_RULE_COUNT; ++r) g_first[r][0] = 0;
  for (int H = 32; H <= kWalkMax; H += 32)
    for (int W = 32; W <= kWalkMax; W += 32)
      for (int li = 0; li < 4; ++li)
        for (int k = 0; k < 4; ++k) {
          const ConvArgs a1 = model_body_conv(1, H, W, li, k);
          const BodyRule r = body_conv_rule(a1, 2);
          const RuleTile t = rule_tile(r);
          if (!g_first[r][0] || (long long)H * W < g_first[r][0]) g_first[r][0] = (long long)H * W, g_first[r][1] = H, g_first[r][2] = W;
          // no intended fall-through: frames under 128 rows are given conv_h3 by the rule itself
          for (int B : {1, 2}) {
            const ConvArgs a = model_body_conv(B, H, W, li, k);
            if (FRESH(conv_shape_check(a, EPI_STD, SFA_MATH_FP16X3)) != SFA_OK) continue;  // a batch run in passes
            unsigned grid = 0;
            const int rc = rule_check(a, body_conv_rule(a, 2), &grid);
            EXPECT(rc == SFA_OK, "%d x %d x %d layer%d conv %d: %s refused by its check (%s)", B, H, W, li + 1, k, body_rule_name(r), g_err);
            // split-K strips: one ticket word per output tile in the model's array (model.hip plan_bufs)
            const long long tick_words = (long long)((B * (H / 32) * (W / 32) + 63) / 64) * (512 / 64);
            if (rc == SFA_OK && t.fam == 1 && t.ks == 2)
              EXPECT(grid / 2 <= tick_words, "%d x %d x %d layer%d conv %d: %u tiles, %lld ticket words", B, H, W, li + 1, k, grid / 2, tick_words);
          }
          EXPECT(t.fam != 0 && t.ks == (t.fam == 3 && (a1.Kpad / 32) % 2 ? 1 : pick_ksplit(a1)), "%d x %d layer%d conv %d: %s", H, W, li + 1, k, body_rule_name(r));
          EXPECT(strip_tile_bn(a1) == (t.fam == 1 ? t.BN : 0), "%d x %d layer%d conv %d: strip_tile_bn %d, rule %s", H, W, li + 1, k,
                 strip_tile_bn(a1), body_rule_name(r));
          EXPECT(body_conv_rule(model_body_conv(181, H, W, li, k), 2) == r, "%d x %d layer%d conv %d: the rule depends on the batch", H, W, li + 1, k);
          // the block operator's launch of the same conv takes the same rule
          const int ih = (H / 4) >> (li > 0 ? li - 1 : 0), iw = (W / 4) >> (li > 0 ? li - 1 : 0);
          const int bh = k < 2 ? ih : ih / (li > 0 ? 2 : 1), bw = k < 2 ? iw : iw / (li > 0 ? 2 : 1);
          for (int B : {1, 2})
            EXPECT(body_conv_rule(block_body_conv(B, bh, bw, li, k >> 1, k & 1), 2) == r, "%d x %d layer%d conv %d: block_forward takes another rule", H,
                   W, li + 1, k);
          // the one-product mode shares the table
          EXPECT(body_conv_rule(a1, 1) == r, "%d x %d layer%d conv %d: SFA_MATH_FP16 takes another rule", H, W, li + 1, k);
        }
}

// conv_plan_check --rules: "layer block conv H W -> rule" for the sixteen body convs at every input H x W (multiples of
// 32 up to 2048); --block layer block B h w: the same two lines for block_forward on a B x h x w map.
static int dump_rules() {
  for (int H = 32; H <= kWalkMax; H += 32)
    for (int W = 32; W <= kWalkMax; W += 32)
      for (int li = 0; li < 4; ++li)
        for (int k = 0; k < 4; ++k)
          std::printf("%d %d %d %d %d -> %s\n", li + 1, k >> 1, (k & 1) + 1, H, W, body_rule_name(body_conv_rule(model_body_conv(1, H, W, li, k), 2)));
  return 0;
}

static int dump_block(int layer, int block, int B, int h, int w) {
  if (layer < 1 || layer > 4 || block < 0 || block > 1 || B < 1 || h < 1 || w < 1) return 2;
  for (int c = 0; c < 2; ++c)
    std::printf("%d %d %d %d %d -> %s\n", layer, block, c + 1, h, w, body_rule_name(body_conv_rule(block_body_conv(B, h, w, layer - 1, block, c), 2)));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "--rules")) return dump_rules();
  if (argc >= 7 && (argc - 2) % 5 == 0 && !std::strcmp(argv[1], "--block")) {
    for (int i = 2; i < argc; i += 5)
      if (int rc = dump_block(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), std::atoi(argv[i + 4]))) return rc;
    return 0;
  }
  if (argc != 1) return 2;
  check_body_rules();
  for (int r = 1; r < BODY_RULE_COUNT; ++r)
    if (g_first[r][0]) std::printf("body rule %-18s first at %lld x %lld\n", body_rule_name((BodyRule)r), g_first[r][1], g_first[r][2]);
    else std::printf("body rule %-18s not reached up to %d x %d\n", body_rule_name((BodyRule)r), kWalkMax, kWalkMax);
  check_make_seg();
  check_families();
  check_stem_chunks();
  check_product();
  check_fast_div();
  std::printf("conv_plan_check: %lld checks, %lld bad\n", g_checks, g_bad);
  return g_bad != 0;
}
