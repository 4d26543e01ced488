// The state layout and the weight pack: the descriptor checks, the layout and size entries, and the two drivers of
// one description of the pack (the units of pack_plan.h, the element rules of pack_row.h).  sfa_pack_weights(_ex)
// walks the units on the host (pack_host.h); sfa_pack_weights_device(_ex) launches one kernel per unit
// (pack_kernel.h) from the state tensors where they live into the packed buffer a model handle reads, the same
// bytes.  The device form is stream-ordered: no host synchronisation, no allocation, no memset node; capturable in
// a HIP graph (the pointers travel by value in the kernel arguments).
#include "pack_host.h"
#include "pack_kernel.h"

#include "dispatch.h"

namespace sfa {

int check_arch(const sfa_arch* a, int backbone) {
  SFA_CHECK_ARG(a != nullptr, "arch is null");
  if (a->num_layers != 18) {
    set_error("only %s is implemented (got %d layers)", backbone == SFA_BACKBONE_DECONV ? "resnet_18" : "fpn_resnet_18",
              a->num_layers);
    return SFA_E_UNSUPPORTED;
  }
  if (a->head_conv != 64) {
    set_error("only head_conv = 64 is implemented (got %d)", a->head_conv);
    return SFA_E_UNSUPPORTED;
  }
  SFA_CHECK_ARG(a->num_heads >= 1 && a->num_heads <= SFA_MAX_HEADS, "num_heads %d out of range",
                a->num_heads);
  for (int j = 0; j < a->num_heads; ++j) {
    SFA_CHECK_ARG(a->head_channels[j] >= 1 && a->head_channels[j] <= 4,
                  "head %d: channels %d out of [1, 4]", j, a->head_channels[j]);
    SFA_CHECK_ARG(strnlen(a->head_names[j], 32) > 0 && strnlen(a->head_names[j], 32) < 32,
                  "head %d: bad name", j);
  }
  return SFA_OK;
}

// The extended descriptor: the base checks of its family; reserved words zero, a known backbone.
int check_arch_ex(const sfa_arch_ex* x) {
  SFA_CHECK_ARG(x != nullptr, "arch is null");
  SFA_CHECK_ARG(x->backbone == SFA_BACKBONE_KFPN || x->backbone == SFA_BACKBONE_DECONV, "unknown backbone %d",
                x->backbone);
  for (int r : x->reserved) SFA_CHECK_ARG(r == 0, "sfa_arch_ex.reserved must be zero");
  return check_arch(&x->base, x->backbone);
}

static int state_entry(const sfa_arch* arch, int backbone, int index, char* name, int name_len, int64_t* shape4,
                       int* ndim) {
  SFA_CHECK_ARG(shape4 && ndim, "state_entry: null argument");
  const auto v = state_layout(arch, backbone);
  SFA_CHECK_ARG(index >= 0 && index < (int)v.size(), "state index %d out of range", index);
  const Entry& e = v[index];
  SFA_CHECK_ARG(name && name_len > (int)e.name.size(), "name buffer too small");
  memcpy(name, e.name.c_str(), e.name.size() + 1);
  for (int i = 0; i < 4; ++i) shape4[i] = i < (int)e.shape.size() ? e.shape[i] : 0;
  *ndim = (int)e.shape.size();
  return SFA_OK;
}

static size_t state_floats_of(const sfa_arch* arch, int backbone) {
  size_t n = 0;
  for (const auto& e : state_layout(arch, backbone))
    if (!is_batches_tracked(e)) n += numel(e);
  return n;
}

// Every unit against what both drivers index (pack_plan.h pack_unit_fits), before either writes anything.
static int check_units(const char* who, const std::vector<PackUnit>& units, const std::vector<Entry>& layout) {
  for (const PackUnit& u : units)
    if (!pack_unit_fits(u, layout)) {
      set_error("%s: a pack unit does not fit the kernel (Kpad %d, rows %d)", who, u.Kpad, u.rows);
      return SFA_E_UNSUPPORTED;
    }
  return SFA_OK;
}

static int pack_weights(const sfa_arch* arch, int backbone, const float* state, size_t state_floats, float* packed) {
  SFA_CHECK_ARG(state && packed, "pack: null argument");
  SFA_CHECK_ARG(state_floats == state_floats_of(arch, backbone), "pack: expected %zu state floats, got %zu",
                state_floats_of(arch, backbone), state_floats);
  const std::vector<Entry> layout = state_layout(arch, backbone);
  const std::vector<PackUnit> units = pack_units(arch, backbone);
  if (int rc = check_units("pack", units, layout)) return rc;
  pack_host(units, pack_sources(layout, state).data(), make_plan(arch, backbone).total, packed);
  return SFA_OK;
}

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
  if (int rc = check_units("pack_device", units, layout)) return rc;
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

// The layout / size / pack entry points: the sfa_arch forms are the SFA_BACKBONE_KFPN case of the sfa_arch_ex forms
// (one implementation each, by family).
extern "C" int sfa_state_count(const sfa_arch* arch) {
  if (check_arch(arch) != SFA_OK) return -1;
  return (int)state_layout(arch).size();
}

extern "C" int sfa_state_count_ex(const sfa_arch_ex* x) {
  if (check_arch_ex(x) != SFA_OK) return -1;
  return (int)state_layout(&x->base, x->backbone).size();
}

extern "C" int sfa_state_entry(const sfa_arch* arch, int index, char* name, int name_len,
                               int64_t* shape4, int* ndim) {
  int rc = check_arch(arch);
  if (rc != SFA_OK) return rc;
  return state_entry(arch, SFA_BACKBONE_KFPN, index, name, name_len, shape4, ndim);
}

extern "C" int sfa_state_entry_ex(const sfa_arch_ex* x, int index, char* name, int name_len, int64_t* shape4,
                                  int* ndim) {
  int rc = check_arch_ex(x);
  if (rc != SFA_OK) return rc;
  return state_entry(&x->base, x->backbone, index, name, name_len, shape4, ndim);
}

extern "C" size_t sfa_state_floats(const sfa_arch* arch) {
  if (check_arch(arch) != SFA_OK) return 0;
  return state_floats_of(arch, SFA_BACKBONE_KFPN);
}

extern "C" size_t sfa_state_floats_ex(const sfa_arch_ex* x) {
  if (check_arch_ex(x) != SFA_OK) return 0;
  return state_floats_of(&x->base, x->backbone);
}

extern "C" size_t sfa_packed_floats(const sfa_arch* arch) {
  if (check_arch(arch) != SFA_OK) return 0;
  return make_plan(arch).total;
}

extern "C" size_t sfa_packed_floats_ex(const sfa_arch_ex* x) {
  if (check_arch_ex(x) != SFA_OK) return 0;
  return make_plan(&x->base, x->backbone).total;
}

extern "C" int sfa_pack_weights(const sfa_arch* arch, const float* state, size_t state_floats,
                                float* packed) {
  int rc = check_arch(arch);
  if (rc != SFA_OK) return rc;
  return pack_weights(arch, SFA_BACKBONE_KFPN, state, state_floats, packed);
}

extern "C" int sfa_pack_weights_ex(const sfa_arch_ex* x, const float* state, size_t state_floats, float* packed) {
  int rc = check_arch_ex(x);
  if (rc != SFA_OK) return rc;
  return pack_weights(&x->base, x->backbone, state, state_floats, packed);
}

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
