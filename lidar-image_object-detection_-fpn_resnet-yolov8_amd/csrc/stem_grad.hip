// sfa_model_stem_forward / sfa_model_stem_grad: the stem (models/fpn_resnet.py:179-182: conv1 7x7 / 2 / pad 3, bn1,
// ReLU, MaxPool2d(3, 2, 1)) as an operator on a caller's (B, 3, H, W) image, BatchNorm folded with its running
// statistics as the handle holds it, and its gradients (gfx950; include/sfa_hip.h has the contract).
//   forward   the model's own unfused launches: launch_nchw3_to_nhwc4 with its per-frame max |x| (record zeroed by
//             launch_zero_words), launch_conv (fp16x3, conv1 + shift + ReLU) -> a, launch_maxpool3s2 -> pooled
//   gradient  stem_pool_adjoint_kernel   dA = a > 0 ? pool adjoint of gp : 0, written once to the workspace
//             the shared bias pair (grad_common.hip)  db' (dA)
//             stem_wgrad_kernel + the shared fold   dW' (dA, x)
//             stem_dgrad_kernel          dx = dgrad_2(dA; W'), only when grad_x is wanted
// Every check is made before the first launch; nothing allocates or synchronises.
#include <cstring>

#include "aux_kernels.h"
#include "conv.h"
#include "dispatch.h"
#include "grad_host.h"
#include "stem_grad_host.h"
#include "stem_grad_kernel.h"

using namespace sfa;

namespace {

int stem_level(const char* who, const sfa_model* model, StemLevel* sl) {
  SFA_CHECK_ARG(model, "%s: null model", who);
  if (int rc = model_stem_level(model, sl)) return rc;
  SFA_CHECK_ARG(aligned16(sl->w) && sl->K % 4 == 0, "%s: conv1 is not packed as the kernels read it", who);
  return SFA_OK;
}

}  // namespace

int sfa::launch_stem_pool_adjoint(const StemShape& s, const float* a, const float* gp, float* dA, hipStream_t st) {
  return launch({dim3((unsigned)ceil_div(s.npix_a, 16)), dim3(256), st}, stem_pool_adjoint_kernel, a, gp, dA, s.oh, s.ow,
                s.ph, s.pw, s.npix_a);
}

int sfa::launch_stem_wgrad(const BlockWgrad& g, const StemShape& s, const float* gr, const float* x, float* part,
                           float* dW, hipStream_t st) {
  if (int rc = launch({dim3((unsigned)g.chunks, (unsigned)kSgColTiles), dim3(256), st}, stem_wgrad_kernel, gr, x, part,
                      s.H, s.W, s.oh, s.ow, s.npix_a, g.Kc))
    return rc;
  return launch_wgrad_fold(part, g.chunks, kSgC, kSgK, 1, dW, kSgK, 0, st);
}

int sfa::launch_stem_dgrad(const StemShape& s, const float* gr, const float* Wp, int ldw, float* dx, hipStream_t st) {
  const int passes = ceil_div(s.npix_x, kSgDgradPixels);
  return launch({dim3((unsigned)(passes < kSgDgradMaxBlocks ? passes : kSgDgradMaxBlocks)), dim3(256), st},
                stem_dgrad_kernel, gr, Wp, ldw, dx, s.H, s.W, s.oh, s.ow, s.npix_x);
}

extern "C" size_t sfa_model_stem_forward_workspace_size(const sfa_model* model, int B, int H, int W) {
  StemLevel sl;
  StemForwardPlan plan;
  if (stem_level("stem_forward_workspace_size", model, &sl) != SFA_OK) return 0;
  if (!stem_forward_plan(B, H, W, &plan))
    return refused("stem_forward_workspace_size: B %d x %d x %d is outside the plan's range", B, H, W);
  return plan.total;
}

extern "C" int sfa_model_stem_forward(const sfa_model* model, const float* x, int B, int H, int W, float* a_out,
                                      float* pooled_out, void* workspace, size_t workspace_bytes, void* stream) {
  StemLevel sl;
  StemForwardPlan plan;
  if (int rc = stem_level("stem_forward", model, &sl)) return rc;
  SFA_CHECK_ARG(B > 0 && H > 0 && W > 0, "stem_forward: B %d, H %d, W %d must be positive", B, H, W);
  if (H > kSgMaxSide || W > kSgMaxSide || B > kSgMaxBatch) {
    set_error("stem_forward: H %d, W %d above %d or B %d above %d: the reused launches cannot index them", H, W,
              kSgMaxSide, B, kSgMaxBatch);
    return SFA_E_UNSUPPORTED;
  }
  SFA_CHECK_ARG(stem_forward_plan(B, H, W, &plan), "stem_forward: B %d x %d x %d has a map of 2^31 bytes", B, H, W);
  SFA_CHECK_ARG(x && a_out && pooled_out && workspace, "stem_forward: null argument");
  SFA_CHECK_ARG(all_aligned16({x, a_out, pooled_out, workspace}),
                "stem_forward: the image, the maps and the workspace must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "stem_forward: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  const StemShape& s = plan.s;
  char* ws = reinterpret_cast<char*>(workspace);
  float* xin = reinterpret_cast<float*>(ws + plan.off_xin);
  unsigned* amax = reinterpret_cast<unsigned*>(ws + plan.off_amax);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ConvArgs a;
  memset(&a, 0, sizeof a);
  a.nseg = 1;
  a.Kpad = sl.K;
  a.w = sl.w;
  a.wx = sl.wx;
  a.wh = sl.wh;
  a.winv = sl.winv;
  a.bias = sl.b;
  a.M = s.npix_a;
  a.N = kSgC;
  a.OH = s.oh;
  a.OW = s.ow;
  a.relu = 1;
  a.y = a_out;
  a.amax_in[0] = amax;
  SFA_CHECK_ARG(make_seg(a.seg[0], xin, B, H, W, 4, 7, 2, 3), "stem_forward: the image passes 32-bit byte offsets");
  if (int rc = launch_zero_words(amax, plan.amax_bytes, st)) return rc;
  if (int rc = launch_nchw3_to_nhwc4(x, xin, B, H, W, false, amax, st)) return rc;
  if (int rc = launch_conv(a, EPI_STD, SFA_MATH_FP16X3, st)) return rc;
  return launch_maxpool3s2(a_out, pooled_out, B, s.oh, s.ow, kSgC, st);
}

extern "C" size_t sfa_model_stem_grad_workspace_size(const sfa_model* model, int B, int H, int W, int max_chunk_pixels) {
  StemLevel sl;
  StemGradPlan plan;
  if (stem_level("stem_grad_workspace_size", model, &sl) != SFA_OK) return 0;
  if (!stem_grad_plan(B, H, W, max_chunk_pixels, &plan))
    return refused("stem_grad_workspace_size: B %d x %d x %d, max_chunk_pixels %d is outside the plan's range", B, H, W,
                   max_chunk_pixels);
  return plan.total;
}

extern "C" int sfa_model_stem_grad_chunk_pixels(const sfa_model* model, int B, int H, int W, int max_chunk_pixels) {
  StemLevel sl;
  StemGradPlan plan;
  if (stem_level("stem_grad_chunk_pixels", model, &sl) != SFA_OK) return 0;
  if (!stem_grad_plan(B, H, W, max_chunk_pixels, &plan))
    return refused("stem_grad_chunk_pixels: B %d x %d x %d, max_chunk_pixels %d is outside the plan's range", B, H, W,
                   max_chunk_pixels);
  return plan.wg.Kc;
}

extern "C" int sfa_model_stem_grad(const sfa_model* model, const float* x, const float* a, const float* gp, int B, int H,
                                   int W, float* grad_x, float* const* dparams, int max_chunk_pixels, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  StemLevel sl;
  StemGradPlan plan;
  if (int rc = stem_level("stem_grad", model, &sl)) return rc;
  SFA_CHECK_ARG(B > 0 && H > 0 && W > 0, "stem_grad: B %d, H %d, W %d must be positive", B, H, W);
  SFA_CHECK_ARG(max_chunk_pixels >= 0, "stem_grad: max_chunk_pixels %d is negative", max_chunk_pixels);
  if (H > kSgMaxSide || W > kSgMaxSide || B > kSgMaxBatch) {
    set_error("stem_grad: H %d, W %d above %d or B %d above %d: sizes sfa_model_stem_forward refuses", H, W, kSgMaxSide,
              B, kSgMaxBatch);
    return SFA_E_UNSUPPORTED;
  }
  SFA_CHECK_ARG(stem_grad_plan(B, H, W, max_chunk_pixels, &plan), "stem_grad: B %d x %d x %d has a map of 2^31 bytes", B,
                H, W);
  float* dW = dparams ? dparams[0] : nullptr;
  float* db = dparams ? dparams[1] : nullptr;
  SFA_CHECK_ARG(a && gp && workspace, "stem_grad: null a, gp or workspace");
  SFA_CHECK_ARG(grad_x || dW || db, "stem_grad: no output wanted");
  SFA_CHECK_ARG(x || !dW, "stem_grad: dW' reads x");
  SFA_CHECK_ARG(all_aligned16({x, a, gp, grad_x, dW, db, workspace}), "stem_grad: every buffer must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "stem_grad: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  const StemShape& s = plan.s;
  char* ws = reinterpret_cast<char*>(workspace);
  float* dA = reinterpret_cast<float*>(ws + plan.off_da);
  float* part = reinterpret_cast<float*>(ws + plan.off_part);
  double* bpart = reinterpret_cast<double*>(ws + plan.off_bpart);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);

  if (int rc = launch_stem_pool_adjoint(s, a, gp, dA, st)) return rc;
  if (db)
    if (int rc = launch_bias_grad(plan.bs, dA, nullptr, bpart, db, st)) return rc;
  if (dW)
    if (int rc = launch_stem_wgrad(plan.wg, s, dA, x, part, dW, st)) return rc;
  if (!grad_x) return SFA_OK;
  return launch_stem_dgrad(s, dA, sl.w, sl.K, grad_x, st);
}
