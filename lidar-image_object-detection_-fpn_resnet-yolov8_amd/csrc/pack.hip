// sfa_pack_weights_device(_ex): sfa_pack_weights on the device, from the state tensors where they live into
// the packed buffer a model handle reads, byte for byte (pack_kernel.h; the plan and its units: pack_plan.h).
// Stream-ordered: no host synchronisation, no allocation, no memset node; capturable in a HIP graph (the
// pointers travel by value in the kernel arguments).
#include "pack_kernel.h"

#include "dispatch.h"

namespace sfa {

bool device_memory_covers(const void* p, size_t bytes) {
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  void* base = nullptr;
  size_t range = 0;
  int dev = -1;
  const bool ok =
      p != nullptr && hipGetDevice(&dev) == hipSuccess && hipPointerGetAttributes(&at, p) == hipSuccess &&
      at.type == hipMemoryTypeDevice && at.device == dev &&
      hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &range, const_cast<void*>(p)) == hipSuccess &&
      (size_t)(static_cast<const char*>(p) - static_cast<const char*>(base)) + bytes <= range;
  if (!ok) (void)hipGetLastError();
  return ok;
}

static int pack_weights_device(const sfa_arch* arch, int backbone, const float* const* state, int count,
                               float* packed, void* stream) {
  SFA_CHECK_ARG(state && packed, "pack_device: null argument");
  const std::vector<Entry> layout = state_layout(arch, backbone);
  SFA_CHECK_ARG(count == (int)layout.size(), "pack_device: expected %zu state entries, got %d", layout.size(), count);
  for (int i = 0; i < count; ++i) {
    const Entry& e = layout[i];
    if (is_batches_tracked(e)) {
      SFA_CHECK_ARG(state[i] == nullptr, "pack_device: entry %d (%s) must be null", i, e.name.c_str());
      continue;
    }
    SFA_CHECK_ARG(state[i] != nullptr, "pack_device: entry %d (%s) is null", i, e.name.c_str());
    SFA_CHECK_ARG((reinterpret_cast<uintptr_t>(state[i]) & 3) == 0, "pack_device: entry %d (%s) is not 4-byte aligned",
                  i, e.name.c_str());
    SFA_CHECK_ARG(device_memory_covers(state[i], (size_t)numel(e) * 4),
                  "pack_device: entry %d (%s) is not %lld floats of memory of the current device", i, e.name.c_str(),
                  (long long)numel(e));
  }
  const Plan plan = make_plan(arch, backbone);
  SFA_CHECK_ARG((reinterpret_cast<uintptr_t>(packed) & 15) == 0, "pack_device: packed_device is not 16-byte aligned");
  SFA_CHECK_ARG(device_memory_covers(packed, plan.total * 4),
                "pack_device: packed_device is not %zu floats of memory of the current device", plan.total);
  const std::vector<PackUnit> units = pack_units(arch, backbone);
  for (const PackUnit& u : units) {
    bool ok = u.Kpad % 8 == 0 && u.Kpad <= kPackMaxRow && u.rows > 0 && u.seg[0].w >= 0 && (u.bias >= 0 || u.seg[0].bn[0] >= 0);
    for (int s = 0; s < u.nseg; ++s) {
      const PackSeg& sg = u.seg[s];
      const int last = u.kind == PACK_DECONV ? 4 * sg.I : sg.k_off + (sg.KH * sg.KW - 1) * sg.Cpad + sg.I;
      ok = ok && sg.w >= 0 && sg.I <= sg.Cpad && last <= u.Kpad;
      // every source index of the kernel lies inside the tensor the layout describes
      const int src_rows = u.kind == PACK_DECONV ? u.N : u.O;
      ok = ok && numel(layout[sg.w]) == (int64_t)src_rows * sg.I * sg.KH * sg.KW;
      for (int q = 0; q < 4; ++q) ok = ok && (sg.bn[q] < 0 ? sg.bn[0] < 0 : numel(layout[sg.bn[q]]) == src_rows);
    }
    ok = ok && (u.bias < 0 || numel(layout[u.bias]) == u.O);
    if (!ok) {
      set_error("pack_device: a pack unit does not fit the kernel (Kpad %d, rows %d)", u.Kpad, u.rows);
      return SFA_E_UNSUPPORTED;
    }
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  auto src = [&](int i) { return i < 0 ? nullptr : state[i]; };
  for (const PackUnit& u : units) {
    PackUnitDev d;
    memset(&d, 0, sizeof d);
    for (int s = 0; s < u.nseg; ++s) {
      const PackSeg& sg = u.seg[s];
      d.seg[s] = PackSegDev{src(sg.w), {src(sg.bn[0]), src(sg.bn[1]), src(sg.bn[2]), src(sg.bn[3])},
                            sg.I, sg.KH, sg.KW, sg.Cpad, sg.k_off};
    }
    d.bias = src(u.bias);
    d.w = packed + u.w;
    d.b = packed + u.b;
    d.wx = u.wx == kNoOffset ? nullptr : reinterpret_cast<uint16_t*>(packed + u.wx);
    d.wh = u.wh == kNoOffset ? nullptr : reinterpret_cast<uint16_t*>(packed + u.wh);
    d.winv = u.winv == kNoOffset ? nullptr : packed + u.winv;
    d.kind = u.kind, d.O = u.O, d.rows = u.rows, d.N = u.N, d.Kpad = u.Kpad, d.nseg = u.nseg;
    if (int rc = launch({dim3(u.rows), dim3(kPackThreads), st}, pack_rows_kernel, d)) return rc;
  }
  const auto gaps = pack_gaps(units, plan.total);
  for (size_t g0 = 0; g0 < gaps.size(); g0 += kPackGaps) {
    PackGapsDev g;
    memset(&g, 0, sizeof g);
    for (size_t i = g0; i < gaps.size() && g.count < kPackGaps; ++i, ++g.count) {
      g.at[g.count] = packed + gaps[i].first;
      g.len[g.count] = (int)(gaps[i].second - gaps[i].first);
    }
    if (int rc = launch({dim3(1), dim3(64), st}, pack_gaps_kernel, g)) return rc;
  }
  return SFA_OK;
}

}  // namespace sfa

using namespace sfa;

extern "C" int sfa_pack_weights_device(const sfa_arch* arch, const float* const* state, int count,
                                       float* packed_device, void* stream) {
  int rc = check_arch(arch);
  if (rc != SFA_OK) return rc;
  return pack_weights_device(arch, SFA_BACKBONE_KFPN, state, count, packed_device, stream);
}

extern "C" int sfa_pack_weights_device_ex(const sfa_arch_ex* x, const float* const* state, int count,
                                          float* packed_device, void* stream) {
  int rc = check_arch_ex(x);
  if (rc != SFA_OK) return rc;
  return pack_weights_device(&x->base, x->backbone, state, count, packed_device, stream);
}
