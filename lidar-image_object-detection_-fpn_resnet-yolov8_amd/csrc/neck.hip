// sfa_model_neck_forward / sfa_model_neck_grad: the FPN neck of models/fpn_resnet.py:197-210 as an operator on a
// caller's four backbone maps, and its gradients (gfx950; include/sfa_hip.h has the contract).
//   forward   U l4 (launch_upsample2x, into the workspace), then per stage one neck_fwd_kernel over the two input
//             segments and, for stages 1 and 2, the resize of its output: six launches
//   gradient  per stage, top (stage 3) down: neck_dgrad_kernel on the skip columns (d_l) and on the up columns
//             (+ g of the map below), neck_wgrad_kernel + the shared fold, the shared bias pair (grad_common.hip),
//             bilinear_up2_adjoint_kernel to the stage below.  Stage 1's up half runs after
//             the adjoint, at l4's resolution: U and a 1x1 convolution commute.  Only what a wanted output needs
//             is launched.
// Every check is made before the first launch; nothing allocates or synchronises.
#include "aux_kernels.h"
#include "conv.h"
#include "dispatch.h"
#include "grad_host.h"
#include "neck_kernel.h"

using namespace sfa;

namespace {

int neck_levels(const char* who, const sfa_model* model, FpnLevel fl[3]) {
  SFA_CHECK_ARG(model, "%s: null model", who);
  for (int f = 0; f < 3; ++f) {
    if (int rc = model_fpn_level(model, f, &fl[f])) return rc;
    SFA_CHECK_ARG(fl[f].N == kNkCout[f] && fl[f].K == kNkUp[f] + kNkSkip[f] && aligned16(fl[f].w),
                  "%s: conv_up_level%d is not the (%d, %d) matrix the kernels take", who, f + 1, kNkCout[f],
                  kNkUp[f] + kNkSkip[f]);
  }
  return SFA_OK;
}

float up_scale(int n) { return n > 1 ? (float)(n - 1) / (float)(2 * n - 1) : 0.f; }  // as launch_upsample2x

int fwd(const float* a0, const float* a1, int k0, int k1, const FpnLevel& fl, float* out, int npix, hipStream_t st) {
  return launch({dim3((unsigned)grad_tiles(npix), (unsigned)(fl.N / kGradTile)), dim3(256), st}, neck_fwd_kernel, a0, a1,
                k0, k1, fl.w, fl.b, out, npix, fl.N);
}

// out (npix, N) = [g +] dz W[:, col0 .. col0 + N)
int dgrad(const float* dz, const FpnLevel& fl, int col0, int N, const float* g, float* out, int npix, hipStream_t st) {
  return launch({dim3((unsigned)grad_tiles(npix), (unsigned)(N / kGradTile)), dim3(256), st}, neck_dgrad_kernel, dz,
                fl.w + col0, fl.K, g, out, npix, N, fl.N);
}

// dW[:, col0 .. col0 + n0 + n1) (row stride ldo) = dz^T cat(x0, x1)
int wgrad(const NeckWgrad& g, const float* dz, const float* x0, const float* x1, int n0, int n1, float* part, float* dW,
          int ldo, int col0, hipStream_t st) {
  const dim3 grid((unsigned)g.chunks, (unsigned)(g.cols / kGradTile), (unsigned)(g.rows / kGradTile));
  if (int rc = launch({grid, dim3(256), st}, neck_wgrad_kernel, dz, x0, x1, n0, n1, part, g.npix, g.Kc, g.rows)) return rc;
  return launch_wgrad_fold(part, g.chunks, g.rows, g.cols, 1, dW, ldo, col0, st);
}

// dst (B, H, W, C) = U^T src
int up_adjoint(const float* src, float* dst, int B, int H, int W, int C, hipStream_t st) {
  return launch({dim3((unsigned)ceil_div(B * H * W * (C / 4), 256)), dim3(256), st}, bilinear_up2_adjoint_kernel,
                reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst), B, H, W, C / 4, up_scale(H),
                up_scale(W));
}

}  // namespace

extern "C" int sfa_neck_pixel_tile(void) { return kGradTile; }

extern "C" size_t sfa_model_neck_forward_workspace_size(const sfa_model* model, int B, int h4, int w4) {
  FpnLevel fl[3];
  NeckForwardPlan plan;
  if (neck_levels("neck_forward_workspace_size", model, fl) != SFA_OK) return 0;
  if (!neck_forward_plan(B, h4, w4, &plan))
    return refused("neck_forward_workspace_size: B %d x %d x %d is outside the plan's range", B, h4, w4);
  return plan.total;
}

extern "C" int sfa_model_neck_forward(const sfa_model* model, const float* l1, const float* l2, const float* l3,
                                      const float* l4, int B, int h4, int w4, float* u2, float* u3, float* u4,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  FpnLevel fl[3];
  NeckForwardPlan plan;
  if (int rc = neck_levels("neck_forward", model, fl)) return rc;
  SFA_CHECK_ARG(B > 0 && h4 > 0 && w4 > 0, "neck_forward: B %d, h4 %d, w4 %d must be positive", B, h4, w4);
  SFA_CHECK_ARG(neck_forward_plan(B, h4, w4, &plan), "neck_forward: B %d x %d x %d passes 32-bit byte offsets", B, h4, w4);
  SFA_CHECK_ARG(l1 && l2 && l3 && l4 && u2 && u3 && u4 && workspace, "neck_forward: null argument");
  SFA_CHECK_ARG(all_aligned16({l1, l2, l3, l4, u2, u3, u4, workspace}),
                "neck_forward: the maps and the workspace must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "neck_forward: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  char* ws = reinterpret_cast<char*>(workspace);
  float* up = reinterpret_cast<float*>(ws + plan.off_up);
  float* z1 = reinterpret_cast<float*>(ws + plan.off_z1);
  float* z2 = reinterpret_cast<float*>(ws + plan.off_z2);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (int rc = launch_upsample2x(l4, up, B, h4, w4, 512, st)) return rc;
  if (int rc = fwd(up, l3, 512, 256, fl[0], z1, plan.npix[1], st)) return rc;
  if (int rc = launch_upsample2x(z1, u2, B, 2 * h4, 2 * w4, 256, st)) return rc;
  if (int rc = fwd(u2, l2, 256, 128, fl[1], z2, plan.npix[2], st)) return rc;
  if (int rc = launch_upsample2x(z2, u3, B, 4 * h4, 4 * w4, 128, st)) return rc;
  return fwd(u3, l1, 128, 64, fl[2], u4, plan.npix[3], st);
}

extern "C" size_t sfa_model_neck_grad_workspace_size(const sfa_model* model, int B, int h4, int w4, int max_chunk_pixels) {
  FpnLevel fl[3];
  NeckGradPlan plan;
  if (neck_levels("neck_grad_workspace_size", model, fl) != SFA_OK) return 0;
  if (!neck_grad_plan(B, h4, w4, max_chunk_pixels, &plan))
    return refused("neck_grad_workspace_size: B %d x %d x %d, max_chunk_pixels %d is outside the plan's range", B, h4, w4,
                   max_chunk_pixels);
  return plan.total;
}

extern "C" int sfa_model_neck_grad_chunk_pixels(const sfa_model* model, int f, int B, int h4, int w4, int max_chunk_pixels) {
  FpnLevel fl[3];
  NeckGradPlan plan;
  if (neck_levels("neck_grad_chunk_pixels", model, fl) != SFA_OK) return 0;
  if (f < 1 || f > 3 || !neck_grad_plan(B, h4, w4, max_chunk_pixels, &plan))
    return refused("neck_grad_chunk_pixels: stage %d of B %d x %d x %d, max_chunk_pixels %d is outside the plan's range", f,
                   B, h4, w4, max_chunk_pixels);
  return f == 1 ? (plan.wg[0].Kc > plan.wg[1].Kc ? plan.wg[0].Kc : plan.wg[1].Kc) : plan.wg[f].Kc;
}

extern "C" int sfa_model_neck_grad(const sfa_model* model, const float* l1, const float* l2, const float* l3,
                                   const float* l4, const float* u2, const float* u3, const float* g2, const float* g3,
                                   const float* g4, int B, int h4, int w4, float* d_l1, float* d_l2, float* d_l3,
                                   float* d_l4, float* const* dparams, int max_chunk_pixels, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  FpnLevel fl[3];
  NeckGradPlan plan;
  if (int rc = neck_levels("neck_grad", model, fl)) return rc;
  SFA_CHECK_ARG(B > 0 && h4 > 0 && w4 > 0, "neck_grad: B %d, h4 %d, w4 %d must be positive", B, h4, w4);
  SFA_CHECK_ARG(max_chunk_pixels >= 0, "neck_grad: max_chunk_pixels %d is negative", max_chunk_pixels);
  SFA_CHECK_ARG(neck_grad_plan(B, h4, w4, max_chunk_pixels, &plan), "neck_grad: B %d x %d x %d passes 32-bit byte offsets",
                B, h4, w4);
  float* dW[3] = {nullptr, nullptr, nullptr};
  float* db[3] = {nullptr, nullptr, nullptr};
  for (int f = 0; dparams && f < 3; ++f) dW[f] = dparams[2 * f], db[f] = dparams[2 * f + 1];
  SFA_CHECK_ARG(g4 && workspace, "neck_grad: null g4 or workspace");
  SFA_CHECK_ARG(d_l1 || d_l2 || d_l3 || d_l4 || dW[0] || db[0] || dW[1] || db[1] || dW[2] || db[2],
                "neck_grad: no output wanted");
  SFA_CHECK_ARG((!dW[2] || (u3 && l1)) && (!dW[1] || (u2 && l2)) && (!dW[0] || (l3 && l4)),
                "neck_grad: a weight gradient needs the maps its convolution read (dW3: u3, l1; dW2: u2, l2; dW1: l3, l4)");
  SFA_CHECK_ARG(all_aligned16({l1, l2, l3, l4, u2, u3, g2, g3, g4, d_l1, d_l2, d_l3, d_l4, dW[0], db[0], dW[1], db[1], dW[2],
                               db[2], workspace}),
                "neck_grad: every buffer must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "neck_grad: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  char* ws = reinterpret_cast<char*>(workspace);
  float* du3 = reinterpret_cast<float*>(ws + plan.off_du3);
  float* dz2 = reinterpret_cast<float*>(ws + plan.off_dz2);
  float* du2 = reinterpret_cast<float*>(ws + plan.off_du2);
  float* dz1 = reinterpret_cast<float*>(ws + plan.off_dz1);
  float* dl = reinterpret_cast<float*>(ws + plan.off_dl);
  float* part = reinterpret_cast<float*>(ws + plan.off_part);
  double* bpart = reinterpret_cast<double*>(ws + plan.off_bpart);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int* npix = plan.npix;
  const bool need_dl = d_l4 || dW[0];
  const bool need_dz1 = need_dl || d_l3 || db[0];
  const bool need_dz2 = need_dz1 || d_l2 || dW[1] || db[1];

  // stage 3: dZ3 = g4
  if (d_l1)
    if (int rc = dgrad(g4, fl[2], 128, 64, nullptr, d_l1, npix[3], st)) return rc;
  if (dW[2])
    if (int rc = wgrad(plan.wg[3], g4, u3, l1, 128, 64, part, dW[2], 192, 0, st)) return rc;
  if (db[2])
    if (int rc = launch_bias_grad(plan.bs[2], g4, nullptr, bpart, db[2], st)) return rc;
  if (!need_dz2) return SFA_OK;
  if (int rc = dgrad(g4, fl[2], 0, 128, g3, du3, npix[3], st)) return rc;
  if (int rc = up_adjoint(du3, dz2, B, 4 * h4, 4 * w4, 128, st)) return rc;

  // stage 2
  if (d_l2)
    if (int rc = dgrad(dz2, fl[1], 256, 128, nullptr, d_l2, npix[2], st)) return rc;
  if (dW[1])
    if (int rc = wgrad(plan.wg[2], dz2, u2, l2, 256, 128, part, dW[1], 384, 0, st)) return rc;
  if (db[1])
    if (int rc = launch_bias_grad(plan.bs[1], dz2, nullptr, bpart, db[1], st)) return rc;
  if (!need_dz1) return SFA_OK;
  if (int rc = dgrad(dz2, fl[1], 0, 256, g2, du2, npix[2], st)) return rc;
  if (int rc = up_adjoint(du2, dz1, B, 2 * h4, 2 * w4, 256, st)) return rc;

  // stage 1: the skip half at l3's resolution, the up half at l4's
  if (d_l3)
    if (int rc = dgrad(dz1, fl[0], 512, 256, nullptr, d_l3, npix[1], st)) return rc;
  if (dW[0])
    if (int rc = wgrad(plan.wg[1], dz1, l3, nullptr, 256, 0, part, dW[0], 768, 512, st)) return rc;
  if (db[0])
    if (int rc = launch_bias_grad(plan.bs[0], dz1, nullptr, bpart, db[0], st)) return rc;
  if (!need_dl) return SFA_OK;
  if (int rc = up_adjoint(dz1, dl, B, h4, w4, 256, st)) return rc;
  if (d_l4)
    if (int rc = dgrad(dl, fl[0], 0, 512, nullptr, d_l4, npix[0], st)) return rc;
  if (dW[0])
    if (int rc = wgrad(plan.wg[0], dl, l4, nullptr, 512, 0, part, dW[0], 768, 0, st)) return rc;
  return SFA_OK;
}
