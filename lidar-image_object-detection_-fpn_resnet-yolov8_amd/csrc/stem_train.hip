// sfa_stem_train_forward / sfa_stem_train_grad: the stem (models/fpn_resnet.py:179-182: conv1 7x7 / 2 / pad 3, bn1,
// ReLU, MaxPool2d(3, 2, 1)) with bn1 in training mode, normalised by and differentiated through the statistics of the
// batch (gfx950; include/sfa_hip.h has the contract).  No model handle: the caller passes the raw float32 parameters.
//   forward   stem_w_relayout_kernel -> Wk, stem_conv_fwd_kernel -> z, the block's statistics pair -> (mean, var) and
//             the float32 (s, t), the block's apply with no skip -> a, launch_maxpool3s2 -> pooled
//   gradient  stem_pool_adjoint_kernel -> dY, the block's BatchNorm backward -> dbeta, dgamma, dZ,
//             stem_wgrad_kernel + the shared fold -> dW (dZ, x), stem_w_relayout_kernel -> Wp and
//             stem_dgrad_kernel -> dx = dgrad_2(dZ; W).  Only what a wanted output needs is launched.
// Every check is made before the first launch; nothing allocates or synchronises.
#include "aux_kernels.h"
#include "block_train_host.h"
#include "dispatch.h"
#include "grad_host.h"
#include "stem_grad_host.h"
#include "stem_train_kernel.h"

using namespace sfa;

namespace {

int relayout(const float* W, float* Wk, float* Wp, hipStream_t st) {
  return launch({dim3((unsigned)ceil_div(kSgC * kStWpLd, 256)), dim3(256), st}, stem_w_relayout_kernel, W, Wk, Wp);
}

// The checks the two entries share: SFA_OK, or the code with the error text set.
int check_dims(const char* who, int B, int H, int W, int max_chunk_pixels, double eps) {
  StemShape sh;
  SFA_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: B %d, H %d, W %d must be positive", who, B, H, W);
  SFA_CHECK_ARG(max_chunk_pixels >= 0, "%s: max_chunk_pixels %d is negative", who, max_chunk_pixels);
  SFA_CHECK_ARG(eps >= 0.0 && eps == eps, "%s: eps must not be negative", who);
  const int rc = stem_train_shape(B, H, W, &sh);
  if (rc == 2) {
    set_error("%s: H %d above %d or B %d above %d: the max-pool launch puts them on grid axes", who, H, kStMaxH, B,
              kStMaxBatch);
    return SFA_E_UNSUPPORTED;
  }
  SFA_CHECK_ARG(rc == 0, "%s: B %d x %d x %d has a map of 2^31 bytes", who, B, H, W);
  SFA_CHECK_ARG(sh.npix_a >= 2, "%s: %d value per channel; training-mode BatchNorm needs more than 1", who, sh.npix_a);
  return SFA_OK;
}

}  // namespace

extern "C" size_t sfa_stem_train_forward_workspace_size(int B, int H, int W, int max_chunk_pixels) {
  StemTrainForwardPlan plan;
  if (!stem_train_forward_plan(B, H, W, max_chunk_pixels, &plan))
    return refused("stem_train_forward_workspace_size: B %d x %d x %d, max_chunk_pixels %d is outside the plan's range "
                   "(fewer than 2 values per channel included)",
                   B, H, W, max_chunk_pixels);
  return plan.total;
}

extern "C" size_t sfa_stem_train_grad_workspace_size(int B, int H, int W, int max_chunk_pixels) {
  StemTrainGradPlan plan;
  if (!stem_train_grad_plan(B, H, W, max_chunk_pixels, &plan))
    return refused("stem_train_grad_workspace_size: B %d x %d x %d, max_chunk_pixels %d is outside the plan's range "
                   "(fewer than 2 values per channel included)",
                   B, H, W, max_chunk_pixels);
  return plan.total;
}

extern "C" int sfa_stem_train_chunk_pixels(int which, int B, int H, int W, int max_chunk_pixels) {
  StemTrainGradPlan plan;
  if (which < 0 || which > 1 || !stem_train_grad_plan(B, H, W, max_chunk_pixels, &plan))
    return refused("stem_train_chunk_pixels: item %d at B %d x %d x %d, max_chunk_pixels %d does not exist", which, B, H,
                   W, max_chunk_pixels);
  return which == 1 ? plan.st.pixels : plan.wg.Kc;
}

extern "C" int sfa_stem_train_forward(const float* x, const float* const* params, double eps, int B, int H, int W,
                                      float* z, float* a, float* pooled, float* stats, int max_chunk_pixels,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  StemTrainForwardPlan plan;
  if (int rc = check_dims("stem_train_forward", B, H, W, max_chunk_pixels, eps)) return rc;
  SFA_CHECK_ARG(stem_train_forward_plan(B, H, W, max_chunk_pixels, &plan),
                "stem_train_forward: B %d x %d x %d is outside the plan's range", B, H, W);
  SFA_CHECK_ARG(x && params && z && a && pooled && stats && workspace, "stem_train_forward: null argument");
  const float *Wt = params[0], *gamma = params[1], *beta = params[2];
  SFA_CHECK_ARG(Wt && gamma && beta, "stem_train_forward: a parameter is null");
  SFA_CHECK_ARG(all_aligned16({x, z, a, pooled, stats, workspace, Wt, gamma, beta}),
                "stem_train_forward: every buffer must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "stem_train_forward: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  const StemShape& s = plan.s;
  char* ws = reinterpret_cast<char*>(workspace);
  float* Wk = reinterpret_cast<float*>(ws + plan.off_wk);
  double* spart = reinterpret_cast<double*>(ws + plan.off_spart);
  float* coef = reinterpret_cast<float*>(ws + plan.off_coef);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);

  if (int rc = relayout(Wt, Wk, nullptr, st)) return rc;
  if (int rc = launch({dim3((unsigned)grad_tiles(s.npix_a)), dim3(256), st}, stem_conv_fwd_kernel, x, (const float*)Wk,
                      z, H, W, s.oh, s.ow, s.npix_a))
    return rc;
  if (int rc = launch_bn_train_stats(plan.st, z, gamma, beta, eps, spart, stats, coef, st)) return rc;
  if (int rc = launch_bn_train_apply(s.npix_a, kSgC, z, coef, nullptr, nullptr, nullptr, a, st)) return rc;
  return launch_maxpool3s2(a, pooled, B, s.oh, s.ow, kSgC, st);
}

extern "C" int sfa_stem_train_grad(const float* x, const float* z, const float* a, const float* gp, const float* stats,
                                   const float* const* params, double eps, int B, int H, int W, float* grad_x,
                                   float* const* dparams, int max_chunk_pixels, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  StemTrainGradPlan plan;
  if (int rc = check_dims("stem_train_grad", B, H, W, max_chunk_pixels, eps)) return rc;
  SFA_CHECK_ARG(stem_train_grad_plan(B, H, W, max_chunk_pixels, &plan),
                "stem_train_grad: B %d x %d x %d is outside the plan's range", B, H, W);
  float* dW = dparams ? dparams[0] : nullptr;
  float* dg = dparams ? dparams[1] : nullptr;
  float* db = dparams ? dparams[2] : nullptr;
  SFA_CHECK_ARG(z && a && gp && stats && params && workspace, "stem_train_grad: null z, a, gp, stats, params or workspace");
  // the backward reads the convolution weight and the BatchNorm weight (not the bias)
  const float *Wt = params[0], *gamma = params[1];
  SFA_CHECK_ARG(Wt && gamma, "stem_train_grad: the weight or the gamma is null");
  SFA_CHECK_ARG(grad_x || dW || dg || db, "stem_train_grad: no output wanted");
  SFA_CHECK_ARG(x || !dW, "stem_train_grad: dW reads x");
  SFA_CHECK_ARG(all_aligned16({x, z, a, gp, stats, Wt, gamma, grad_x, dW, dg, db, workspace}),
                "stem_train_grad: every buffer must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "stem_train_grad: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  const StemShape& s = plan.s;
  char* ws = reinterpret_cast<char*>(workspace);
  float* dY = reinterpret_cast<float*>(ws + plan.off_dy);
  float* dZ = reinterpret_cast<float*>(ws + plan.off_dz);
  float* Wp = reinterpret_cast<float*>(ws + plan.off_wp);
  float* part = reinterpret_cast<float*>(ws + plan.off_part);
  double* rpart = reinterpret_cast<double*>(ws + plan.off_rpart);
  double* sums = reinterpret_cast<double*>(ws + plan.off_sums);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);

  // dY = a > 0 ? pool adjoint of gp : 0 is already masked: the BatchNorm backward takes it as it is
  if (int rc = launch_stem_pool_adjoint(s, a, gp, dY, st)) return rc;
  if (int rc = launch_bn_train_backward(plan.st, dY, nullptr, z, stats, gamma, eps, rpart, sums, dg, db,
                                        (grad_x || dW) ? dZ : nullptr, st))
    return rc;
  if (dW)
    if (int rc = launch_stem_wgrad(plan.wg, s, dZ, x, part, dW, st)) return rc;
  if (!grad_x) return SFA_OK;
  if (int rc = relayout(Wt, nullptr, Wp, st)) return rc;
  return launch_stem_dgrad(s, dZ, Wp, kStWpLd, grad_x, st);
}
