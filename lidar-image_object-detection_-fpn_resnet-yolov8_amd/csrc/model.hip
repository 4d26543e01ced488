// FPN-ResNet-18 (KFPN) and plain ResNet-18 (deconv) models: the model handle, its options, the buffer plan and
// the forward orchestration (the state layout and the weight pack: pack.hip).  The two families (sfa_backbone)
// share the stem and the residual layers; what follows layer4 differs.
//
// Reference: models/fpn_resnet.py:112-301 (PoseResNet, BasicBlock, get_pose_net),
//            models/resnet.py:115-284 (the plain PoseResNet: three transposed convs, one head level),
//            models/model_utils.py:25-43 (create_model).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "aux_kernels.h"
#include "conv.h"
#include "conv_plan.h"
#include "pack_plan.h"

namespace sfa {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
}

}  // namespace sfa

using namespace sfa;

// Pre-tiled LDS images (conv_wimage.h) of the convs whose fp16x3 kernel reads its W pieces from one: the
// detection heads' 3x3 convs on conv_r3_kernel<256, 320> (image i = head level i). One device buffer,
// shared by a model and the handles created from it by sfa_model_create_twin.
struct WImages {
  unsigned char* dev = nullptr;
  sfa::WImageGeom geom[sfa::WIMG_MAX];
  sfa::WImagePlan plan;
  ~WImages() {
    if (dev) (void)hipFree(dev);
  }
};

// ... and of the residual layers' 3x3 / stride-1 convs on conv_h3s_kernel (h3sopt::W_IMAGE): a second device
// buffer with a plan of its own, about the size of those convs' fp16 terms again (~25 MB). One image per conv,
// in the strip K order at the tile width its strip instance has at the maps conv.hip gives that instance
// (body_image_bn); a launch that takes another tile width or family reads the packed terms (Fwd::layers).
struct WBodyImages {
  unsigned char* dev = nullptr;
  int index[4][4];  // image of conv k of layer li (Fwd::layers' order), or -1
  size_t wh[sfa::WIMG_BODY_MAX];  // the conv's packed fp16 terms (floats into the packed buffer)
  sfa::WImageGeom geom[sfa::WIMG_BODY_MAX];
  sfa::WBodyImagePlan plan;
  ~WBodyImages() {
    if (dev) (void)hipFree(dev);
  }
};

struct sfa_model {
  sfa_arch arch;
  int backbone = SFA_BACKBONE_KFPN;  // sfa_backbone: what follows layer4
  const float* w;
  Plan plan;
  int math;
  int fpn_commute = 7;  // fp16x3: bit f -> FPN conv f as up(W_a x) + W_b skip (env SFA_FPN_COMMUTE, mask)
  // fp16x3 stem form (env SFA_STEM_PATCH): 1 (default) = the 16 x 16 patch kernel + its merge pass
  // (stem_patch_kernel.h); 0 = the implicit-GEMM stem conv + the max-pool kernel, as the other math
  // modes (the round-4 full-width band stem measured slower: tools/experiments/r04)
  int stem_patch = 1;
  // fp16x3 FPN 1x1 convs on the persistent kernels of fpn_kernel.h, mask (env SFA_FPN_GEMM): bit f =
  // level f's low-resolution W_a . x conv (weight-resident row streaming), bit 3 + f = its skip conv
  // with the upsampled residual (level 2: full rows with the taps from an LDS ring; levels 0 / 1: flat
  // pixel steps, fpn_seg_kernel); the other convs run on conv_h3 / conv_r3 (the same products for the
  // skip convs). Default 61 = the low-res convs of levels 0 and 2 and the three skip convs, the ones
  // measured faster (profiles/r04d_*, r04l_*, r05n_*); 63 (level 1's low-res conv too: -5 us serial, other
  // bits within 2e-5) measured bench-equal
  int fpn_gemm = 61;
  // fp16x3 split-K layer4 strip convs: 1 (default) = the last slice of each tile combines the partials in
  // the conv kernel (tickets, conv_h3_kernel.h splitk_ticket), 0 = splitk_reduce_kernel launches; the
  // same bits (env SFA_SPLITK_TICKETS). conv_h3's split convs keep the reduce launch.
  int splitk_tickets = 1;
  // fp16x3 heads read W from the pre-tiled LDS images (1, env SFA_W_IMAGES) or gather it from the packed
  // row-major terms (0); the same bits. `wimg` is null when the images could not be built (no device, the
  // packed weights not in device memory, another head count): the row-major kernels run.
  int w_images = 1;
  std::shared_ptr<WImages> wimg;
  // the residual layers' strip convs read W from their images (1, env SFA_BODY_W_IMAGES) or from the packed
  // terms (0); the same bits. Both this and w_images must be on. `bimg` is null as `wimg` is.
  int body_w_images = 1;
  std::shared_ptr<WBodyImages> bimg;
  // Side stream for the level-0 heads (they only need up_level2, so they overlap the rest
  // of the FPN and the level-1/2 heads); created with the model on the current device,
  // used only when the forward's stream is on that device.
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr, mid = nullptr;
  int device = -1;
  std::mutex fork_mu;  // fork ... join of one forward is not interleaved with another's
  // Kernel probe (sfa_model_set_probe): timing events around each head-level launch, recorded
  // on the stream that launches it (never while that stream is being captured); PROBE_SERIAL
  // keeps every launch on the caller's stream so each head launch has the chip to itself.
  int probe = 0;
  // (a deconv model: pairs 0..2 around its three transposed convs, pair 3 around its heads launch)
  hipEvent_t probe_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

// The model's side stream(s) and their events, created on the current device; on failure
// (no device) none, and the forward runs every launch on the caller's stream.
static void drop_side_streams(sfa_model* m) {
  for (hipEvent_t* e : {&m->fork, &m->join, &m->mid})
    if (*e) {
      (void)hipEventDestroy(*e);
      *e = nullptr;
    }
  if (m->side) {
    (void)hipStreamDestroy(m->side);
    m->side = nullptr;
  }
}

static void make_side_streams(sfa_model* m) {
  if (hipGetDevice(&m->device) != hipSuccess || hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&m->fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&m->join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&m->mid, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    drop_side_streams(m);
  }
}

// The geometry of head level f's image: the whole 3x3 conv, conv_r3_kernel<256, 320>'s chunk-major K order.
static sfa::WImageGeom head_wimage_geom(const PHeads& hp, int Cin) {
  return sfa::WImageGeom{hp.N, hp.K, hp.K, 0, 320, 2, hp.K / 32, Cin};
}

// The tile width of the strip instance a body conv of N output channels runs on (conv.hip: 64-wide convs and
// the split-K 2 layer4 convs on 128 x 64 tiles, layer2 / 3 on 128-wide tiles).
static int body_image_bn(int N) { return N == 64 || N == 512 ? 64 : 128; }

// (Re)builds the heads' images from the packed weights, on `st`.
static int fill_wimages(const sfa_model* m, hipStream_t st) {
  const WImages& wi = *m->wimg;
  for (int f = 0; f < wi.plan.count; ++f)
    if (int rc = sfa::launch_wimage_build(wi.geom[f], reinterpret_cast<const uint16_t*>(m->w + m->plan.heads[f].wh),
                                          wi.dev + wi.plan.off[f], st))
      return rc;
  return SFA_OK;
}

// ... and the body convs'.
static int fill_body_wimages(const sfa_model* m, hipStream_t st) {
  const WBodyImages& bi = *m->bimg;
  for (int i = 0; i < bi.plan.count; ++i)
    if (int rc = sfa::launch_wimage_build(bi.geom[i], reinterpret_cast<const uint16_t*>(m->w + bi.wh[i]),
                                          bi.dev + bi.plan.off[i], st))
      return rc;
  return SFA_OK;
}

// Allocates and builds the images at create. Only from packed weights that are device memory of the
// current device and cover the plan (a handle over anything else, or created without a device, keeps the
// row-major kernels); built on the null stream and waited for, so a forward on any stream finds them.
static bool weights_on_device(const sfa_model* m) {
  return (reinterpret_cast<uintptr_t>(m->w) & 15) == 0 && sfa::device_memory_covers(m->w, m->plan.total * 4);
}

static void make_wimages(sfa_model* m) {
  if (m->plan.heads[0].N != 320) return;  // the image instance is the five-head 256 x 320 tile
  auto wi = std::make_shared<WImages>();
  const int nlev = m->backbone == SFA_BACKBONE_DECONV ? 1 : 3;
  for (int f = 0; f < nlev; ++f) wi->geom[f] = head_wimage_geom(m->plan.heads[f], kFpnC[f]);
  if (sfa::wimage_plan(wi->geom, nlev, &wi->plan) != nullptr || hipMalloc(&wi->dev, wi->plan.total) != hipSuccess) {
    (void)hipGetLastError();
    wi->dev = nullptr;
    return;
  }
  m->wimg = wi;
  if (fill_wimages(m, nullptr) != SFA_OK || hipStreamSynchronize(nullptr) != hipSuccess) {
    (void)hipGetLastError();
    m->wimg.reset();
  }
}

// The body convs' images: the one-segment 3x3 / stride-1 convs of the residual layers (all four of layer1,
// block 1's two of layers 2 - 4), the ones conv_h3s_kernel runs.
static void make_body_wimages(sfa_model* m) {
  auto bi = std::make_shared<WBodyImages>();
  int n = 0;
  for (int li = 0; li < 4; ++li)
    for (int k = 0; k < 4; ++k) {
      bi->index[li][k] = -1;
      if (li > 0 && k < 2) continue;  // stride 2 / the fused downsample segment
      const PConv& pc = m->plan.blk[li][k >> 1][k & 1];
      const int C = 64 << li;
      if (pc.Kpad != 9 * C || pc.N % body_image_bn(pc.N) != 0) continue;
      bi->index[li][k] = n;
      bi->wh[n] = pc.wh;
      bi->geom[n] = sfa::WImageGeom{pc.N, pc.Kpad, pc.Kpad, 0, body_image_bn(pc.N), 2, 0, C, 1};
      ++n;
    }
  if (sfa::wimage_plan(bi->geom, n, &bi->plan) != nullptr || bi->plan.total == 0 ||
      hipMalloc(&bi->dev, bi->plan.total) != hipSuccess) {
    (void)hipGetLastError();
    bi->dev = nullptr;
    return;
  }
  m->bimg = bi;
  if (fill_body_wimages(m, nullptr) != SFA_OK || hipStreamSynchronize(nullptr) != hipSuccess) {
    (void)hipGetLastError();
    m->bimg.reset();
  }
}

extern "C" int sfa_abi_version(void) { return SFA_ABI_VERSION; }
extern "C" const char* sfa_last_error_string(void) { return g_err.c_str(); }

static int model_create(const sfa_arch* arch, int backbone, const float* packed_device, sfa_model** out,
                        const sfa_model* twin_of = nullptr) {
  SFA_CHECK_ARG(packed_device && out, "model_create: null argument");
  sfa_model* m = new sfa_model;
  m->arch = *arch;
  m->backbone = backbone;
  m->w = packed_device;
  m->plan = make_plan(arch, backbone);
  m->math = SFA_MATH_FP16X3;
  // A/B convenience: the environment seeds the options once, here (sfa_model_set_option
  // overrides them; nothing reads the environment on the launch path)
  if (const char* e = getenv("SFA_STEM_PATCH")) m->stem_patch = atoi(e) != 0;
  if (const char* e = getenv("SFA_FPN_COMMUTE")) m->fpn_commute = atoi(e) & 7;
  if (const char* e = getenv("SFA_FPN_GEMM")) m->fpn_gemm = atoi(e) & 63;
  if (const char* e = getenv("SFA_SPLITK_TICKETS")) m->splitk_tickets = atoi(e) != 0;
  if (const char* e = getenv("SFA_W_IMAGES")) m->w_images = atoi(e) != 0;
  if (const char* e = getenv("SFA_BODY_W_IMAGES")) m->body_w_images = atoi(e) != 0;
  if (twin_of) {
    m->wimg = twin_of->wimg;  // the same weights: the same images
    m->bimg = twin_of->bimg;
  } else if (weights_on_device(m)) {
    make_wimages(m);
    make_body_wimages(m);
  }
  bool side_streams = true;  // env SFA_SIDE_STREAMS=0: every launch on the caller's stream (A/B)
  if (const char* e = getenv("SFA_SIDE_STREAMS")) side_streams = strcmp(e, "0") != 0;
  // the deconv family has no parallel branch: no side streams, every launch on the caller's stream
  if (side_streams && backbone == SFA_BACKBONE_KFPN) make_side_streams(m);
  *out = m;
  return SFA_OK;
}

extern "C" int sfa_model_create(const sfa_arch* arch, const float* packed_device, sfa_model** out) {
  int rc = check_arch(arch);
  if (rc != SFA_OK) return rc;
  return model_create(arch, SFA_BACKBONE_KFPN, packed_device, out);
}

extern "C" int sfa_model_create_ex(const sfa_arch_ex* x, const float* packed_device, sfa_model** out) {
  int rc = check_arch_ex(x);
  if (rc != SFA_OK) return rc;
  return model_create(&x->base, x->backbone, packed_device, out);
}

extern "C" int sfa_model_create_twin(const sfa_model* model, sfa_model** out) {
  SFA_CHECK_ARG(model && out, "create_twin: null argument");
  return model_create(&model->arch, model->backbone, model->w, out, model);
}

extern "C" int sfa_model_refresh_weight_images(sfa_model* model, void* stream) {
  SFA_CHECK_ARG(model, "refresh_weight_images: null model");
  int rc = SFA_OK;  // (no images: nothing derived from the weights)
  if (model->wimg) rc = fill_wimages(model, reinterpret_cast<hipStream_t>(stream));
  if (rc == SFA_OK && model->bimg) rc = fill_body_wimages(model, reinterpret_cast<hipStream_t>(stream));
  return rc;
}

extern "C" size_t sfa_model_weight_image_bytes(const sfa_model* model) {
  return model && model->wimg ? model->wimg->plan.total : 0;
}

extern "C" size_t sfa_model_body_weight_image_bytes(const sfa_model* model) {
  return model && model->bimg ? model->bimg->plan.total : 0;
}

extern "C" void sfa_model_destroy(sfa_model* model) {
  if (!model) return;
  for (hipEvent_t e : model->probe_ev)
    if (e) (void)hipEventDestroy(e);
  drop_side_streams(model);
  delete model;
}

extern "C" int sfa_model_set_side_streams(sfa_model* model, int on) {
  SFA_CHECK_ARG(model, "set_side_streams: null model");
  if (model->backbone == SFA_BACKBONE_DECONV) return SFA_OK;  // no parallel branch: nothing to switch
  std::lock_guard<std::mutex> lk(model->fork_mu);
  if (!on && model->side) {
    // the side streams' last forward must be done before they go (the caller's stream has
    // joined them, so nothing enqueued later depends on them)
    SFA_HIP_TRY(hipStreamSynchronize(model->side));
    drop_side_streams(model);
  } else if (on && !model->side) {
    make_side_streams(model);
    SFA_CHECK_ARG(model->side, "set_side_streams: no side stream could be created on this device");
  }
  return SFA_OK;
}

extern "C" int sfa_model_set_option(sfa_model* model, int key, int value) {
  SFA_CHECK_ARG(model, "set_option: null model");
  std::lock_guard<std::mutex> lk(model->fork_mu);
  switch (key) {
    case SFA_OPT_STEM_PATCH:
      SFA_CHECK_ARG(value == 0 || value == 1, "set_option: STEM_PATCH %d not 0 / 1", value);
      model->stem_patch = value;
      break;
    case SFA_OPT_FPN_COMMUTE:
      SFA_CHECK_ARG(value >= 0 && value <= 7, "set_option: FPN_COMMUTE mask %d not in 0..7", value);
      model->fpn_commute = value;
      break;
    case SFA_OPT_FPN_GEMM:
      SFA_CHECK_ARG(value >= 0 && value <= 63, "set_option: FPN_GEMM mask %d not in 0..63", value);
      model->fpn_gemm = value;
      break;
    case SFA_OPT_SPLITK_TICKETS:
      SFA_CHECK_ARG(value == 0 || value == 1, "set_option: SPLITK_TICKETS %d not 0 / 1", value);
      model->splitk_tickets = value;
      break;
    case SFA_OPT_W_IMAGES:
      SFA_CHECK_ARG(value == 0 || value == 1, "set_option: W_IMAGES %d not 0 / 1", value);
      model->w_images = value;
      break;
    case SFA_OPT_BODY_W_IMAGES:
      SFA_CHECK_ARG(value == 0 || value == 1, "set_option: BODY_W_IMAGES %d not 0 / 1", value);
      model->body_w_images = value;
      break;
    default: set_error("set_option: unknown key %d", key); return SFA_E_INVALID;
  }
  return SFA_OK;
}

extern "C" int sfa_model_get_option(const sfa_model* model, int key, int* value) {
  SFA_CHECK_ARG(model && value, "get_option: null argument");
  switch (key) {
    case SFA_OPT_STEM_PATCH: *value = model->stem_patch; break;
    case SFA_OPT_FPN_COMMUTE: *value = model->fpn_commute; break;
    case SFA_OPT_FPN_GEMM: *value = model->fpn_gemm; break;
    case SFA_OPT_SPLITK_TICKETS: *value = model->splitk_tickets; break;
    case SFA_OPT_W_IMAGES: *value = model->w_images; break;
    case SFA_OPT_BODY_W_IMAGES: *value = model->body_w_images; break;
    default: set_error("get_option: unknown key %d", key); return SFA_E_INVALID;
  }
  return SFA_OK;
}

extern "C" int sfa_model_set_math(sfa_model* model, int math) {
  SFA_CHECK_ARG(model, "set_math: null model");
  SFA_CHECK_ARG(math == SFA_MATH_F32 || math == SFA_MATH_BF16X6 || math == SFA_MATH_FP16X3 || math == SFA_MATH_FP16,
                "set_math: unknown mode %d", math);
  if (model->backbone == SFA_BACKBONE_DECONV && math != SFA_MATH_FP16X3) {
    set_error("set_math: the resnet_18 (deconv) model runs SFA_MATH_FP16X3 only: its transposed convolutions have "
              "no f32 / bf16x6 kernel, and its SFA_MATH_FP16 error is not yet budgeted (mode %d refused)", math);
    return SFA_E_UNSUPPORTED;
  }
  model->math = math;
  return SFA_OK;
}

extern "C" int sfa_model_get_math(const sfa_model* model) { return model ? model->math : -1; }

extern "C" int sfa_model_set_probe(sfa_model* model, int flags) {
  SFA_CHECK_ARG(model, "set_probe: null model");
  SFA_CHECK_ARG((flags & ~(SFA_PROBE_HEADS | SFA_PROBE_SERIAL)) == 0, "set_probe: unknown flags %d", flags);
  if (flags & SFA_PROBE_HEADS)
    for (hipEvent_t& e : model->probe_ev)
      if (!e) SFA_HIP_TRY(hipEventCreate(&e));
  model->probe = flags;
  return SFA_OK;
}

extern "C" int sfa_model_probe_times(const sfa_model* model, float* ms, int n) {
  SFA_CHECK_ARG(model && ms && n >= 0 && n <= (model->backbone == SFA_BACKBONE_DECONV ? 4 : 3),
                "probe_times: bad arguments");
  SFA_CHECK_ARG(model->probe & SFA_PROBE_HEADS, "probe_times: probe not enabled");
  for (int f = 0; f < n; ++f) {
    SFA_HIP_TRY(hipEventSynchronize(model->probe_ev[2 * f + 1]));
    SFA_HIP_TRY(hipEventElapsedTime(&ms[f], model->probe_ev[2 * f], model->probe_ev[2 * f + 1]));
  }
  return SFA_OK;
}

namespace sfa {

// Activation buffers of one forward (NHWC f32), carved from the workspace.
struct Bufs {
  size_t xin, s0, p0, t[4], a[4], l[4], up1, c1, up2, c2, up3, up4, L0, L1, L2, amax, tick, tick_words, part,
      part_floats, total;
  size_t d[3];  // deconv family: the three transposed convs' outputs (up1 .. up4, L1, L2 unused)
};

// fp16x3 activation maxima (conv.h): per tensor a conv reads (named by its producer), B
// frames of SFA_AMAX_WORDS words.  Pooling and bilinear upsampling never raise max |x|, so their
// outputs share their input's slot.
enum AmaxSlot { AM_INPUT = 0, AM_STEM = 1, AM_BLK = 2 /* + 4 li + 2 bi + ci */, AM_FPN = 18,
                AM_DECONV = 18 /* deconv family, + layer */, AM_COUNT = 21 };

static Bufs plan_bufs(const sfa_arch* arch, int backbone, int B, int H, int W) {
  Bufs b;
  memset(&b, 0, sizeof b);
  size_t cur = 0;
  auto take = [&](size_t floats) {
    const size_t o = cur;
    cur = align_up(cur + floats * 4, 256);
    return o;
  };
  const size_t P2 = (size_t)(H / 2) * (W / 2), P4 = (size_t)(H / 4) * (W / 4);
  b.xin = take((size_t)B * H * W * 4);
  b.s0 = take((size_t)B * P2 * 64);
  b.p0 = take((size_t)B * P4 * 64);
  for (int li = 0; li < 4; ++li) {
    const size_t px = (size_t)(H >> (li + 2)) * (W >> (li + 2));
    const size_t n = (size_t)B * px * (64 << li);
    b.t[li] = take(n);
    b.a[li] = take(n);
    b.l[li] = take(n);
  }
  const size_t P8 = (size_t)(H / 8) * (W / 8), P16 = (size_t)(H / 16) * (W / 16);
  int nch = 0;
  for (int j = 0; j < arch->num_heads; ++j) nch += arch->head_channels[j];
  if (backbone == SFA_BACKBONE_DECONV) {
    b.d[0] = take((size_t)B * P16 * 256);
    b.d[1] = take((size_t)B * P8 * 256);
    b.d[2] = take((size_t)B * P4 * 256);
    b.L0 = take((size_t)nch * B * P4);  // the one head level, channel-planar, at (H/4, W/4)
  } else {
    b.up1 = take((size_t)B * P16 * 512);
    b.c1 = take((size_t)B * P16 * 256);
    b.up2 = take((size_t)B * P8 * 256);
    b.c2 = take((size_t)B * P8 * 128);
    b.up3 = take((size_t)B * P4 * 128);
    b.up4 = take((size_t)B * P4 * 64);
    b.L0 = take((size_t)nch * B * P8);
    b.L1 = take((size_t)nch * B * P4);
    b.L2 = take((size_t)nch * B * P4);
  }
  // the activation maxima and the split-K tickets (one zeroing memset per forward, right after them)
  b.amax = take((size_t)AM_COUNT * B * SFA_AMAX_WORDS);
  // split-K tickets (conv_h3_kernel.h splitk_ticket): one word per output tile of each of the four
  // layer4 convs, for tiles of >= 64 x 64
  b.tick_words = (size_t)((B * (H / 32) * (W / 32) + 63) / 64) * (512 / 64);
  b.tick = take(4 * b.tick_words);
  // split-K partial sums (conv.hip pick_ksplit: 2 slices of the 512-wide layer4 convs)
  b.part_floats = (size_t)2 * B * (H / 32) * (W / 32) * 512;
  b.part = take(b.part_floats);
  b.total = cur;
  return b;
}

static ConvSeg seg(const float* x, int B, int H, int W, int C, int k, int stride, int pad) {
  ConvSeg g;
  make_seg(g, x, B, H, W, C, k, stride, pad);  // oversize inputs are rejected by launch_conv
  return g;
}

static ConvArgs conv_args(const float* wbase, const PConv& pc, int B, int OH, int OW, float* y,
                          const float* res, int relu) {
  ConvArgs a;
  memset(&a, 0, sizeof a);
  a.nseg = 1;
  a.Kpad = pc.Kpad;
  a.w = wbase + pc.w;
  a.wx = reinterpret_cast<const uint16_t*>(wbase + pc.wx);
  a.wh = reinterpret_cast<const uint16_t*>(wbase + pc.wh);
  a.winv = wbase + pc.winv;
  a.bias = wbase + pc.b;
  a.res = res;
  a.y = y;
  a.M = B * OH * OW;
  a.N = pc.N;
  a.OH = OH;
  a.OW = OW;
  a.relu = relu;
  return a;
}

}  // namespace sfa

// Frames one forward pass runs at once (sfa_forward_max_batch): every conv kernel reads its input
// segments through buffer resources with 32-bit byte offsets (conv.hip launch_conv: < 2 GiB). The
// widest conv input per frame is up_level3 / the level-1 heads' input, (H/4)(W/4) x 128 floats =
// 32 H W bytes (the stem input, 12-16 H W bytes, and every other map are smaller), so a pass holds
// floor((2^31 - 1) / (32 H W)) frames: 181 at 608 x 608. Larger batches run in passes of that
// many frames (sfa_model_forward); frames are independent and their arithmetic batch-invariant
// (per-frame fp16x3 scales), so the chunking changes no bit.  Deconv family: the widest conv input is
// the heads' 256-channel (H/4)(W/4) map, 64 H W bytes per frame: 90 frames at 608 x 608.
static int forward_max_batch(int H, int W, int backbone = SFA_BACKBONE_KFPN) {
  if (H <= 0 || W <= 0) return 0;
  const unsigned long long per_frame =
      (backbone == SFA_BACKBONE_DECONV ? 64ull : 32ull) * (unsigned long long)H * (unsigned long long)W;
  const unsigned long long n = ((1ull << 31) - 1) / per_frame;
  return n > 0x7fffffffull ? 0x7fffffff : (int)n;
}

extern "C" int sfa_forward_max_batch(int height, int width) { return forward_max_batch(height, width); }

extern "C" int sfa_model_forward_max_batch(const sfa_model* m, int height, int width) {
  return m ? forward_max_batch(height, width, m->backbone) : 0;
}

extern "C" size_t sfa_forward_workspace_size(const sfa_model* m, int batch, int height, int width) {
  if (!m || batch <= 0 || height <= 0 || width <= 0) return 0;
  const int bmax = forward_max_batch(height, width, m->backbone);
  if (bmax < 1) return 0;
  return plan_bufs(&m->arch, m->backbone, std::min(batch, bmax), height, width).total;
}

extern "C" int64_t sfa_forward_buffer_offset(const sfa_model* m, int batch, int height, int width,
                                             int which) {
  if (!m || batch <= 0 || height <= 0 || width <= 0) return -1;
  const int bmax = forward_max_batch(height, width, m->backbone);
  if (bmax < 1) return -1;
  const Bufs b = plan_bufs(&m->arch, m->backbone, std::min(batch, bmax), height, width);
  const bool deconv = m->backbone == SFA_BACKBONE_DECONV;
  if (deconv ? (which >= SFA_BUF_UP_LEVEL2 && which <= SFA_BUF_HEADS_L2)
             : (which >= SFA_BUF_DECONV1 && which <= SFA_BUF_DECONV3))
    return -1;  // the other family's maps
  switch (which) {
    case SFA_BUF_LAYER1: return (int64_t)b.l[0];
    case SFA_BUF_LAYER2: return (int64_t)b.l[1];
    case SFA_BUF_LAYER3: return (int64_t)b.l[2];
    case SFA_BUF_LAYER4: return (int64_t)b.l[3];
    case SFA_BUF_UP_LEVEL2: return (int64_t)b.up2;
    case SFA_BUF_UP_LEVEL3: return (int64_t)b.up3;
    case SFA_BUF_UP_LEVEL4: return (int64_t)b.up4;
    case SFA_BUF_HEADS_L0: return (int64_t)b.L0;
    case SFA_BUF_HEADS_L1: return (int64_t)b.L1;
    case SFA_BUF_HEADS_L2: return (int64_t)b.L2;
    case SFA_BUF_DECONV1: return (int64_t)b.d[0];
    case SFA_BUF_DECONV2: return (int64_t)b.d[1];
    case SFA_BUF_DECONV3: return (int64_t)b.d[2];
    default: return -1;
  }
}

// The head parameters of KFPN level `level` inside the handle (conv.h HeadsLevel).
int sfa::model_heads_level(const sfa_model* m, int level, HeadsLevel* out) {
  if (m->backbone == SFA_BACKBONE_DECONV) {
    set_error("heads_grad: a SFA_BACKBONE_DECONV model has no KFPN head levels");
    return SFA_E_UNSUPPORTED;
  }
  SFA_CHECK_ARG(level >= 0 && level < 3, "heads_grad: level %d outside 0..2", level);
  const PHeads& hp = m->plan.heads[level];
  out->w3 = m->w + hp.w3;
  out->b3 = m->w + hp.b3;
  out->w1 = m->w + hp.w1;
  out->b1 = m->w + hp.b1;
  out->wh = reinterpret_cast<const uint16_t*>(m->w + hp.wh);
  out->winv = m->w + hp.winv;
  out->Cin = kFpnC[level];
  out->num_heads = m->arch.num_heads;
  for (int j = 0; j < SFA_MAX_HEADS; ++j) out->ch[j] = j < m->arch.num_heads ? m->arch.head_channels[j] : 0;
  return SFA_OK;
}

// conv_up_level{f + 1} inside the handle (conv.h FpnLevel).
int sfa::model_fpn_level(const sfa_model* m, int f, FpnLevel* out) {
  if (m->backbone == SFA_BACKBONE_DECONV) {
    set_error("neck: a SFA_BACKBONE_DECONV model has no FPN neck");
    return SFA_E_UNSUPPORTED;
  }
  SFA_CHECK_ARG(f >= 0 && f < 3, "neck: stage %d outside 0..2", f);
  const PConv& pc = m->plan.fpn[f];
  SFA_CHECK_ARG(pc.Kpad == pc.K, "neck: conv_up_level%d is packed with padded rows", f + 1);
  out->w = m->w + pc.w;
  out->b = m->w + pc.b;
  out->N = pc.N;
  out->K = pc.K;
  return SFA_OK;
}

// layer{layer}.{block} inside the handle (conv.h BlockLevel).
int sfa::model_block_level(const sfa_model* m, int layer, int block, BlockLevel* out) {
  if (m->backbone == SFA_BACKBONE_DECONV) {
    set_error("block: the gradients of a SFA_BACKBONE_DECONV model's blocks are not covered");
    return SFA_E_UNSUPPORTED;
  }
  SFA_CHECK_ARG(layer >= 1 && layer <= 4 && block >= 0 && block <= 1, "block: layer%d.%d outside layer1..4, block 0..1",
                layer, block);
  for (int c = 0; c < 2; ++c) {
    const PConv& pc = m->plan.blk[layer - 1][block][c];
    SFA_CHECK_ARG(pc.Kpad == pc.K, "block: layer%d.%d conv%d is packed with padded rows", layer, block, c + 1);
    out->w[c] = m->w + pc.w;
    out->b[c] = m->w + pc.b;
    out->winv[c] = m->w + pc.winv;
    out->wx[c] = reinterpret_cast<const uint16_t*>(m->w + pc.wx);
    out->wh[c] = reinterpret_cast<const uint16_t*>(m->w + pc.wh);
    out->K[c] = pc.K;
  }
  out->cout = 64 << (layer - 1);
  out->downsample = block == 0 && layer > 1;
  out->cin = out->downsample ? out->cout / 2 : out->cout;
  out->stride = out->downsample ? 2 : 1;
  out->kds = 9 * out->cout;
  return SFA_OK;
}

// conv1 + bn1 inside the handle (conv.h StemLevel).
int sfa::model_stem_level(const sfa_model* m, StemLevel* out) {
  const PConv& pc = m->plan.stem;
  SFA_CHECK_ARG(pc.N == 64 && pc.K == 196 && pc.Kpad >= pc.K, "stem: conv1 is not packed as 64 rows of 7 x 7 x 4");
  out->w = m->w + pc.w;
  out->b = m->w + pc.b;
  out->winv = m->w + pc.winv;
  out->wx = reinterpret_cast<const uint16_t*>(m->w + pc.wx);
  out->wh = reinterpret_cast<const uint16_t*>(m->w + pc.wh);
  out->K = pc.Kpad;
  return SFA_OK;
}

#define SFA_RC(expr)            \
  do {                          \
    int rc_ = (expr);           \
    if (rc_ != SFA_OK) return rc_; \
  } while (0)

namespace sfa {

// A map that a conv reads: NHWC (B, h, w, c) and the amax slot of its producer.
struct Map {
  const float* x;
  int h, w, c, slot;
};

static int blk_slot(int li, int bi, int ci) { return AM_BLK + 4 * li + 2 * bi + ci; }

// One level of the FPN top-down path (Pass::fpn_row).
struct FpnRow {
  Map lo;         // the low-resolution input
  float* up;      // lo upsampled x2: what the concat form reads
  float* lo_out;  // W_a . lo at the low resolution: what the commuted form adds, upsampled, in its epilogue
  Map skip;       // the skip map, at twice lo's dims
  float* out;
  int out_slot;
};

// One forward pass over B frames: what its stages share, and the stages in the order they run.
struct Pass {
  const sfa_model* m;
  const float* wb;
  const Plan& p;
  const Bufs bf;
  char* ws;
  hipStream_t st;  // the caller's stream
  int B, H, W;
  // fp16x3: every conv input's max |x| is recorded by its producer (slots zeroed by forward_pass)
  // SFA_MATH_FP16: the fp16x3 plumbing (scales, amax words, tickets, patch stem, commuted FPN) with one
  // product per MAC in the body convs and the heads; the stem and the FPN convs stay fp16x3 (math_sf)
  bool h3;
  int math_sf;

  Pass(const sfa_model* model, int B_, int H_, int W_, void* workspace, void* stream)
      : m(model), wb(model->w), p(model->plan), bf(plan_bufs(&model->arch, model->backbone, B_, H_, W_)),
        ws(reinterpret_cast<char*>(workspace)), st(reinterpret_cast<hipStream_t>(stream)), B(B_), H(H_), W(W_),
        h3(model->math == SFA_MATH_FP16X3 || model->math == SFA_MATH_FP16),
        math_sf(model->math == SFA_MATH_FP16 ? SFA_MATH_FP16X3 : model->math) {}

  float* F(size_t off) const { return reinterpret_cast<float*>(ws + off); }
  unsigned* AM(int slot) const {
    return h3 ? reinterpret_cast<unsigned*>(ws + bf.amax) + (size_t)slot * B * SFA_AMAX_WORDS : nullptr;
  }
  // split-K tickets of the layer4 convs (the only split ones, conv.hip pick_ksplit): the slice that
  // finishes last combines the partials in the conv kernel (no reduce launch); fp16x3 only
  unsigned* TK(int li, int ci) const {
    return h3 && li == 3 && m->splitk_tickets ? reinterpret_cast<unsigned*>(ws + bf.tick) + (size_t)ci * bf.tick_words
                                              : nullptr;
  }
  void io(ConvArgs& a, int in0, int in1, int out) const {
    a.amax_in[0] = in0 >= 0 ? AM(in0) : nullptr;
    a.amax_in[1] = in1 >= 0 ? AM(in1) : nullptr;
    a.amax_out = out >= 0 ? AM(out) : nullptr;
    a.part = F(bf.part);
    a.part_floats = bf.part_floats;
  }

  // Timing events 2 pair, 2 pair + 1 around one launch on stream s (sfa_model_set_probe), never while s
  // is being captured.
  template <class Launch>
  int probed(int pair, hipStream_t s, Launch launch) const {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool probe = (m->probe & SFA_PROBE_HEADS) && hipStreamIsCapturing(s, &cap) == hipSuccess &&
                       cap == hipStreamCaptureStatusNone;
    if (probe) SFA_HIP_TRY(hipEventRecord(m->probe_ev[2 * pair], s));
    SFA_RC(launch());
    if (probe) SFA_HIP_TRY(hipEventRecord(m->probe_ev[2 * pair + 1], s));
    return SFA_OK;
  }

  // stem conv7x7/s2/p3 + BN + ReLU (fpn_resnet.py:179-181) + max-pool (:182) -> p0
  int stem(const float* x, int in_layout) const {
    const int H2 = H / 2, W2 = W / 2;
    // The patch stem (fp16x3) reads the caller's layout itself, scales every tile by its own max |x|
    // and max-pools in its epilogue: no layout conversion, no input amax pass, no max-pool launch
    // (stem_patch_kernel.h).
    const bool patch_stem = h3 && m->stem_patch && H2 % 16 == 0 && W2 % 16 == 0;
    const float* xin = x;
    if (patch_stem) {
    } else if (in_layout != SFA_IN_NHWC4) {
      SFA_RC(launch_nchw3_to_nhwc4(x, F(bf.xin), B, H, W, in_layout == SFA_IN_NCHW3_FLIP_HW, AM(AM_INPUT), st));
      xin = F(bf.xin);
    } else if (h3) {
      SFA_RC(launch_amax_nhwc4(x, B, H, W, AM(AM_INPUT), st));
    }
    ConvArgs a = conv_args(wb, p.stem, B, H2, W2, patch_stem ? F(bf.p0) : F(bf.s0), nullptr, 1);
    a.seg[0] = seg(xin, B, H, W, 4, 7, 2, 3);  // the patch stem reads NCHW3 planes through it too
    io(a, AM_INPUT, -1, AM_STEM);
    if (patch_stem) {  // the tile-border cells' parts go through a side buffer and a merge pass
      a.amax_in[0] = nullptr;  // per-tile scales
      a.stem_in = in_layout == SFA_IN_NHWC4 ? STEM_IN_NHWC4
                                             : (in_layout == SFA_IN_NCHW3_FLIP_HW ? STEM_IN_NCHW3_FLIP : STEM_IN_NCHW3);
      a.part = F(bf.s0);  // the (here unused) unfused stem buffer
      a.part_floats = (size_t)B * H2 * W2 * 64;
      return launch_stem_patch(a, st);
    }
    SFA_RC(launch_conv(a, EPI_STD, math_sf, st));
    return launch_maxpool3s2(F(bf.s0), F(bf.p0), B, H2, W2, 64, st);
  }

  // residual layers (fpn_resnet.py:184-187), p0 -> l[0..3]. Per layer, block 0: conv1 (stride), conv2 + the
  // block's input (li > 0: through the fused 1x1 / stride-2 downsample, a second K-segment); block 1: conv1,
  // conv2 + block 0's output. Conv k's ticket index and output slot are k.
  int layers() const {
    Map x = {F(bf.p0), H / 4, W / 4, 64, AM_STEM};  // maxpool keeps the stem's max
    for (int li = 0; li < 4; ++li) {
      const int planes = 64 << li, stride = li == 0 ? 1 : 2;
      const int oh = x.h / stride, ow = x.w / stride;
      float *t = F(bf.t[li]), *av = F(bf.a[li]), *lv = F(bf.l[li]);
      const struct {
        Map in;
        int stride;
        float* y;
        const float* res;
        bool downsample;  // x as the second segment
      } convs[4] = {{x, stride, t, nullptr, false},
                    {{t, oh, ow, planes, blk_slot(li, 0, 0)}, 1, av, li == 0 ? x.x : nullptr, li > 0},
                    {{av, oh, ow, planes, blk_slot(li, 0, 1)}, 1, t, nullptr, false},
                    {{t, oh, ow, planes, blk_slot(li, 1, 0)}, 1, lv, av, false}};
      for (int k = 0; k < 4; ++k) {
        const auto& cv = convs[k];
        ConvArgs a = conv_args(wb, p.blk[li][k >> 1][k & 1], B, oh, ow, cv.y, cv.res, 1);
        a.seg[0] = seg(cv.in.x, B, cv.in.h, cv.in.w, cv.in.c, 3, cv.stride, 1);
        if (cv.downsample) {
          a.nseg = 2;
          a.kseg1 = 9 * planes;
          a.seg[1] = seg(x.x, B, x.h, x.w, x.c, 1, stride, 0);
        }
        io(a, cv.in.slot, cv.downsample ? x.slot : -1, blk_slot(li, k >> 1, k & 1));
        a.tile_cnt = TK(li, k);
        a.tile_cnt_words = (int)bf.tick_words;
        // the conv's pre-tiled W image, when this launch takes the strip instance of the image's tile width
        // (fp16x3: conv.hip reads it, the other modes do not)
        if (m->w_images && m->body_w_images && m->bimg && m->bimg->index[li][k] >= 0) {
          const WBodyImages& bi = *m->bimg;
          const int i = bi.index[li][k];
          if (strip_tile_bn(a) == bi.geom[i].BN) {
            a.wimg = bi.dev + bi.plan.off[i];
            a.wimg_bytes = (unsigned)bi.plan.bytes[i];
            a.wimg_bn = bi.geom[i].BN;
          }
        }
        SFA_RC(launch_conv(a, EPI_STD, m->math, st));
      }
      x = {lv, oh, ow, planes, blk_slot(li, 1, 1)};
    }
    return SFA_OK;
  }

  // Where each head's channels sit in a channel-planar level block, and the caller's buffers.
  KfpnOut head_layout(float* const* head_out) const {
    KfpnOut ko;
    memset(&ko, 0, sizeof ko);
    for (int j = 0; j < m->arch.num_heads; ++j) {
      ko.ptr[j] = head_out[j];
      ko.ch[j] = m->arch.head_channels[j];
      ko.off[j] = ko.total_ch;
      ko.total_ch += ko.ch[j];
    }
    ko.num_heads = m->arch.num_heads;
    return ko;
  }

  // Detection heads (fpn_resnet.py:219-233): all heads of one level in one launch, conv3x3 -> ReLU ->
  // conv1x1 fused, into the channel-planar block `out`.
  ConvArgs head_args(const Map& in, const PHeads& hp, const KfpnOut& ko, float* out) const {
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.nseg = 1;
    a.seg[0] = seg(in.x, B, in.h, in.w, in.c, 3, 1, 1);
    a.Kpad = hp.K;
    a.w = wb + hp.w3;
    a.wx = reinterpret_cast<const uint16_t*>(wb + hp.wx);
    a.wh = reinterpret_cast<const uint16_t*>(wb + hp.wh);
    a.winv = wb + hp.winv;
    a.amax_in[0] = AM(in.slot);
    a.bias = wb + hp.b3;
    a.M = B * in.h * in.w;
    a.N = hp.N;
    a.OH = in.h;
    a.OW = in.w;
    a.relu = 1;
    a.hw1 = wb + hp.w1;
    a.hb1 = wb + hp.b1;
    for (int j = 0; j < ko.num_heads; ++j) {
      a.hch[j] = ko.ch[j];
      a.hoff[j] = ko.off[j];
    }
    a.hout = out;
    if (m->w_images && m->wimg) {  // this level's pre-tiled W image (fp16x3: conv.hip reads it, the other modes do not)
      const int f = (int)(&hp - p.heads);
      a.wimg = m->wimg->dev + m->wimg->plan.off[f];
      a.wimg_bytes = (unsigned)m->wimg->plan.bytes[f];
    }
    return a;
  }

  // Plain resnet_18 (resnet.py:230-234): three ConvTranspose2d(4, s2, p1) + BN + ReLU, layer4 ->
  // (H/4, W/4, 256), one launch each (deconv_h3_kernel.h); then every head in one fused launch (the KFPN
  // level-0 heads kernel's shape) into a channel-planar block, and its relayout into the caller's per-head
  // buffers.  All on the caller's stream; probe pairs 0..2 around the transposed convs, 3 around the heads.
  int deconv_tail(float* const* head_out) const {
    Map x = {F(bf.l[3]), H / 32, W / 32, 512, blk_slot(3, 1, 1)};
    for (int i = 0; i < 3; ++i) {
      const PDeconv& pd = p.dec[i];
      DeconvArgs d;
      memset(&d, 0, sizeof d);
      d.x = x.x;
      d.H = x.h;
      d.W = x.w;
      d.C = pd.C;
      d.logC = ilog2(pd.C);
      d.bytes = (unsigned)((size_t)B * x.h * x.w * pd.C * 4);  // <= 16 H W bytes per frame: inside the pass limit
      d.wh = reinterpret_cast<const uint16_t*>(wb + pd.wh);
      d.winv = wb + pd.winv;
      d.bias = wb + pd.b;
      d.amax_in = AM(x.slot);
      d.amax_out = AM(AM_DECONV + i);
      d.y = F(bf.d[i]);
      d.M = B * x.h * x.w;
      d.N = pd.N;
      d.K = pd.K;
      SFA_RC(probed(i, st, [&] { return launch_deconv(d, B, st); }));
      x = {F(bf.d[i]), 2 * x.h, 2 * x.w, pd.N, AM_DECONV + i};
    }
    const KfpnOut ko = head_layout(head_out);
    const ConvArgs a = head_args(x, p.heads[0], ko, F(bf.L0));
    SFA_RC(probed(3, st, [&] { return launch_conv(a, EPI_HEAD, m->math, st); }));
    return launch_heads_relayout(F(bf.L0), ko, B, x.h, x.w, st);
  }

  // FPN top-down (fpn_resnet.py:197-210), level f = conv_up_level(f + 1) over cat(up(lo), skip).
  FpnRow fpn_row(int f) const {
    const int H16 = H / 16, W16 = W / 16, H8 = H / 8, W8 = W / 8;
    float* lo1 = F(bf.up1) + (size_t)B * (H / 32) * (W / 32) * 256;  // the three lo_out share up1's buffer
    const FpnRow rows[3] = {
        {{F(bf.l[3]), H / 32, W / 32, 512, blk_slot(3, 1, 1)}, F(bf.up1), F(bf.up1),
         {F(bf.l[2]), H16, W16, 256, blk_slot(2, 1, 1)}, F(bf.c1), AM_FPN + 0},
        {{F(bf.c1), H16, W16, 256, AM_FPN + 0}, F(bf.up2), lo1,
         {F(bf.l[1]), H8, W8, 128, blk_slot(1, 1, 1)}, F(bf.c2), AM_FPN + 1},
        {{F(bf.c2), H8, W8, 128, AM_FPN + 1}, F(bf.up3), lo1 + (size_t)B * H16 * W16 * 128,
         {F(bf.l[0]), H / 4, W / 4, 64, blk_slot(0, 1, 1)}, F(bf.up4), AM_FPN + 2}};
    return rows[f];
  }

  // One FPN level on stream fs. Concat form: bilinear x2 (align_corners) + channel concat, read by the
  // 1x1 conv as two K-segments (no concat buffer).
  // Commuted form (fp16x3, m->fpn_commute bit f): the conv runs as two convs on K-slices of its packed
  // weights, W_a up(x) + W_b skip + b = up(W_a x) + W_b skip + b (bilinear resize and a 1x1 conv commute;
  // the interpolation weights sum to 1): W_a x at the LOW resolution into a half-res buffer (no bias),
  // then W_b skip + b with that buffer added bilinearly upsampled in the epilogue. A quarter of W_a's
  // MACs, and up_level1 is never materialised.
  int fpn_level(int f, hipStream_t fs) const {
    const FpnRow r = fpn_row(f);
    const PConv& pc = p.fpn[f];
    ConvArgs a = conv_args(wb, pc, B, r.skip.h, r.skip.w, r.out, nullptr, 0);
    if (!(h3 && ((m->fpn_commute >> f) & 1))) {
      // levels 1 and 2 find lo upsampled already (their heads' input); level 0's has no other reader
      if (f == 0) SFA_RC(launch_upsample2x(r.lo.x, r.up, B, r.lo.h, r.lo.w, r.lo.c, fs));
      a.nseg = 2;
      a.kseg1 = r.lo.c;
      a.seg[0] = seg(r.up, B, r.skip.h, r.skip.w, r.lo.c, 1, 1, 0);
      a.seg[1] = seg(r.skip.x, B, r.skip.h, r.skip.w, r.skip.c, 1, 1, 0);
      io(a, r.lo.slot, r.skip.slot, r.out_slot);
      return launch_conv(a, EPI_STD, math_sf, fs);
    }
    {
      ConvArgs lo = conv_args(wb, pc, B, r.lo.h, r.lo.w, r.lo_out, nullptr, 0);
      lo.bias = nullptr;
      lo.Kpad = r.lo.c;
      lo.wstride = pc.Kpad;
      lo.wk0 = 0;
      lo.seg[0] = seg(r.lo.x, B, r.lo.h, r.lo.w, r.lo.c, 1, 1, 0);
      lo.fpn_gemm = (m->fpn_gemm >> f) & 1;
      io(lo, r.lo.slot, -1, -1);
      SFA_RC(launch_conv(lo, EPI_STD, math_sf, fs));
    }
    a.Kpad = r.skip.c;
    a.wstride = pc.Kpad;
    a.wk0 = r.lo.c;
    a.seg[0] = seg(r.skip.x, B, r.skip.h, r.skip.w, r.skip.c, 1, 1, 0);
    a.res_up = r.lo_out;
    a.res_sh = r.lo.h > 1 ? (float)(r.lo.h - 1) / (float)(2 * r.lo.h - 1) : 0.f;
    a.res_sw = r.lo.w > 1 ? (float)(r.lo.w - 1) / (float)(2 * r.lo.w - 1) : 0.f;
    a.fpn_gemm = (m->fpn_gemm >> (3 + f)) & 1;
    io(a, r.skip.slot, -1, r.out_slot);
    return launch_conv(a, EPI_STD, math_sf, fs);
  }

  // The heads of KFPN level f on stream hs; probe pair f.
  int launch_heads(int f, const KfpnOut& ko, hipStream_t hs) const {
    const Map in[3] = {{F(bf.up2), H / 8, W / 8, kFpnC[0], AM_FPN + 0},  // up_level2 / 3 / 4, from
                       {F(bf.up3), H / 4, W / 4, kFpnC[1], AM_FPN + 1},  // conv_up_level1 / 2 / 3
                       {F(bf.up4), H / 4, W / 4, kFpnC[2], AM_FPN + 2}};
    float* out[3] = {F(bf.L0), F(bf.L1), F(bf.L2)};
    const ConvArgs a = head_args(in[f], p.heads[f], ko, out[f]);
    return probed(f, hs, [&] { return launch_conv(a, EPI_HEAD, m->math, hs); });
  }

  // What runs between the fork and the join, with up_level2 written. The level-0 heads need only that, so
  // they go to the side stream; level 2 (needs up_level4) follows them there and level 1 runs here: the
  // two 1,444-tile launches run side by side, so neither one's last partial wave of tiles leaves CUs idle.
  // Without a side stream: heads 0, FPN, heads 1, heads 2 on the caller's stream.
  int forked_section(const KfpnOut& ko, hipStream_t side) const {
    SFA_RC(launch_heads(0, ko, side ? side : st));
    SFA_RC(fpn_level(1, st));
    SFA_RC(launch_upsample2x(F(bf.c2), F(bf.up3), B, H / 8, W / 8, 128, st));
    SFA_RC(fpn_level(2, st));
    if (side) {
      SFA_HIP_TRY(hipEventRecord(m->mid, st));
      SFA_HIP_TRY(hipStreamWaitEvent(side, m->mid, 0));
      SFA_RC(launch_heads(2, ko, side));
    }
    SFA_RC(launch_heads(1, ko, st));
    if (!side) SFA_RC(launch_heads(2, ko, st));
    return SFA_OK;
  }

  // Fork the side stream off the caller's, run forked_section, join. Two invariants, both carried by this
  // function's shape:
  //  * fork_mu is taken before m->side is read and held until after the join: sfa_model_set_side_streams
  //    destroys the stream under the same lock, so a concurrent call cannot pull it out from under this
  //    forward, and one forward's fork ... join is not interleaved with another's;
  //  * the join runs whatever forked_section returns: a failure inside leaves a graph capture valid (it
  //    follows the event edges) and no work orphaned on the side stream.
  int fork_join_heads(const KfpnOut& ko) const {
    std::lock_guard<std::mutex> fork_lock(const_cast<sfa_model*>(m)->fork_mu);
    int sdev = -1;
    const bool overlap = m->side && !(m->probe & SFA_PROBE_SERIAL) && hipStreamGetDevice(st, &sdev) == hipSuccess &&
                         sdev == m->device;
    if (overlap) {
      SFA_HIP_TRY(hipEventRecord(m->fork, st));
      SFA_HIP_TRY(hipStreamWaitEvent(m->side, m->fork, 0));
    }
    const int rc = forked_section(ko, overlap ? m->side : nullptr);
    if (overlap) {
      SFA_HIP_TRY(hipEventRecord(m->join, m->side));
      SFA_HIP_TRY(hipStreamWaitEvent(st, m->join, 0));
    }
    return rc;
  }

  // KFPN: FPN level 0 and its upsample, the three head levels around FPN levels 1 and 2, apply_kfpn
  // (fpn_resnet.py:248-254).
  int kfpn_tail(float* const* head_out) const {
    const KfpnOut ko = head_layout(head_out);
    SFA_RC(fpn_level(0, st));
    SFA_RC(launch_upsample2x(F(bf.c1), F(bf.up2), B, H / 16, W / 16, 256, st));
    SFA_RC(fork_join_heads(ko));
    return launch_kfpn(F(bf.L0), F(bf.L1), F(bf.L2), ko, B, H / 4, W / 4, st);
  }
};

}  // namespace sfa

// One pass over B <= forward_max_batch(H, W) frames (arguments checked by sfa_model_forward).
static int forward_pass(const sfa_model* m, const float* x, int in_layout, int B, int H, int W,
                        float* const* head_out, void* workspace, void* stream) {
  const Pass c(m, B, H, W, workspace, stream);
  if (c.h3)  // the amax words and the split-K tickets after them
    SFA_RC(launch_zero_words(c.ws + c.bf.amax, c.bf.tick + 4 * c.bf.tick_words * 4 - c.bf.amax, c.st));
  SFA_RC(c.stem(x, in_layout));
  SFA_RC(c.layers());
  return m->backbone == SFA_BACKBONE_DECONV ? c.deconv_tail(head_out) : c.kfpn_tail(head_out);
}

extern "C" int sfa_model_forward(const sfa_model* m, const float* x, int in_layout, int B, int H,
                                 int W, float* const* head_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  SFA_CHECK_ARG(m && x && head_out && workspace, "forward: null argument");
  SFA_CHECK_ARG(B >= 1 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0,
                "forward: input (%d, 3, %d, %d) must have H, W multiples of 32", B, H, W);
  SFA_CHECK_ARG(in_layout == SFA_IN_NCHW3 || in_layout == SFA_IN_NHWC4 ||
                    in_layout == SFA_IN_NCHW3_FLIP_HW,
                "forward: bad layout");
  const int bmax = forward_max_batch(H, W, m->backbone);
  if (bmax < 1) {
    set_error("forward: one %d x %d frame exceeds the conv kernels' 32-bit buffer offsets", H, W);
    return SFA_E_UNSUPPORTED;
  }
  const int bc = std::min(B, bmax);
  const size_t need = plan_bufs(&m->arch, m->backbone, bc, H, W).total;
  if (workspace_bytes < need) {
    set_error("forward: workspace %zu < required %zu bytes", workspace_bytes, need);
    return SFA_E_WORKSPACE;
  }
  for (int j = 0; j < m->arch.num_heads; ++j) SFA_CHECK_ARG(head_out[j], "forward: null head out");
  // batches above the per-pass limit run as consecutive passes of bc frames on the caller's stream,
  // sharing the workspace (stream order serialises them)
  const size_t in_frame = (size_t)(in_layout == SFA_IN_NHWC4 ? 4 : 3) * H * W;
  const size_t out_px = (size_t)(H / 4) * (W / 4);
  float* outs[SFA_MAX_HEADS];
  for (int f0 = 0; f0 < B; f0 += bc) {
    const int nb = std::min(bc, B - f0);
    for (int j = 0; j < m->arch.num_heads; ++j)
      outs[j] = head_out[j] + (size_t)f0 * m->arch.head_channels[j] * out_px;
    SFA_RC(forward_pass(m, x + (size_t)f0 * in_frame, in_layout, nb, H, W, outs, workspace, stream));
  }
  return SFA_OK;
}
