// sfa_block_train_forward / sfa_block_train_grad: one BasicBlock of layer1..4 (models/fpn_resnet.py:42-71) with its
// BatchNorms in training mode, normalised by and differentiated through the statistics of the batch (gfx950;
// include/sfa_hip.h has the contract).  No model handle: the caller passes the raw float32 parameters.
//   forward   per convolution: block_w_relayout_kernel, block_conv_fwd_kernel -> z, bn_stats_kernel + fold ->
//             (mean, var) and the float32 (s, t); bn_apply_kernel -> mid, and -> y with the skip
//   gradient  per BatchNorm: bn_bwd_reduce_kernel + fold -> dbeta, dgamma, bn_bwd_apply_kernel -> dZ;
//             block_kernel.h's weight gradients over dZ2 / dZd / dZ1 and data gradients (dA with mid's mask in the
//             epilogue; dx with the identity skip's masked gy in the epilogue or dZd as the second K segment)
//             Only what a wanted output needs is launched.
// Every check is made before the first launch; nothing allocates or synchronises.
#include <cstring>

#include "block_host.h"
#include "block_train_host.h"
#include "block_train_kernel.h"
#include "dispatch.h"
#include "grad_host.h"

using namespace sfa;

namespace {

int relayout(const float* W, int cout, int cin, int taps, float* Wk, float* Wt, hipStream_t st) {
  return launch({dim3((unsigned)ceil_div(cout * taps * cin, 256)), dim3(256), st}, block_w_relayout_kernel, W, cout, cin,
                taps, Wk, Wt);
}

// z = conv(x; W) and the statistics + (s, t) of the BatchNorm after it
int conv_bn(const BlockShape& s, const GradBias& sb, const float* x, const float* W, const float* gamma,
            const float* beta, double eps, int cin, int h, int w, int stride, int tap0, int ntaps, float* Wk, float* z,
            double* spart, float* stats, float* coef, hipStream_t st) {
  if (int rc = relayout(W, s.cout, cin, ntaps, Wk, nullptr, st)) return rc;
  const BkConvFwd t = {x, Wk, h, w, s.oh, s.ow, stride, cin, s.cout, tap0, ntaps, s.npix_out};
  if (int rc = launch({dim3((unsigned)grad_tiles(s.npix_out), (unsigned)(s.cout / kGradTile)), dim3(256), st},
                      block_conv_fwd_kernel, t, z))
    return rc;
  return launch_bn_train_stats(sb, z, gamma, beta, eps, spart, stats, coef, st);
}

int apply(const BlockShape& s, const float* z, const float* c, const float* x, const float* zd, const float* cd,
          float* out, hipStream_t st) {
  return launch_bn_train_apply(s.npix_out, s.cout, z, c, x, zd, cd, out, st);
}

// The backward of one BatchNorm: dbeta, dgamma (each may be null) and, when dz is not null, dZ.
int bn_backward(const BlockShape&, const GradBias& sb, const float* g, const float* gm, const float* z,
                const float* stats, const float* gamma, double eps, double* rpart, double* sums, float* dgamma,
                float* dbeta, float* dz, hipStream_t st) {
  return launch_bn_train_backward(sb, g, gm, z, stats, gamma, eps, rpart, sums, dgamma, dbeta, dz, st);
}

}  // namespace

int sfa::launch_bn_train_stats(const GradBias& sb, const float* z, const float* gamma, const float* beta, double eps,
                               double* spart, float* stats, float* coef, hipStream_t st) {
  const unsigned cy = (unsigned)ceil_div(sb.cout, 256);
  if (int rc = launch({dim3((unsigned)sb.blocks, cy), dim3(256), st}, bn_stats_kernel, z, spart, sb.npix, sb.pixels,
                      sb.cout))
    return rc;
  return launch({dim3(cy), dim3(256), st}, bn_stats_fold_kernel, (const double*)spart, sb.blocks, sb.cout, sb.npix, gamma,
                beta, eps, stats, coef);
}

int sfa::launch_bn_train_apply(int npix, int cout, const float* z, const float* coef, const float* x, const float* zd,
                               const float* cd, float* out, hipStream_t st) {
  const int quads = npix * cout / 4;
  return launch({dim3((unsigned)ceil_div(quads, 256)), dim3(256), st}, bn_apply_kernel, z, coef, x, zd, cd, out, quads,
                cout);
}

int sfa::launch_bn_train_backward(const GradBias& sb, const float* g, const float* gm, const float* z,
                                  const float* stats, const float* gamma, double eps, double* rpart, double* sums,
                                  float* dgamma, float* dbeta, float* dz, hipStream_t st) {
  const unsigned cy = (unsigned)ceil_div(sb.cout, 256);
  if (int rc = launch({dim3((unsigned)sb.blocks, cy), dim3(256), st}, bn_bwd_reduce_kernel, g, gm, z, stats, rpart,
                      sb.npix, sb.pixels, sb.cout))
    return rc;
  if (int rc = launch({dim3(cy), dim3(256), st}, bn_bwd_fold_kernel, (const double*)rpart, sb.blocks, sb.cout, stats, eps,
                      sums, dgamma, dbeta))
    return rc;
  if (!dz) return SFA_OK;
  const int total = sb.npix * sb.cout;
  return launch({dim3((unsigned)ceil_div(total, 256)), dim3(256), st}, bn_bwd_apply_kernel, g, gm, z, stats, gamma,
                (const double*)sums, eps, sb.npix, total, sb.cout, dz);
}

extern "C" size_t sfa_block_train_forward_workspace_size(int layer, int block, int B, int h, int w,
                                                         int max_chunk_pixels) {
  BlockTrainForwardPlan plan;
  if (!block_train_forward_plan(layer, block, B, h, w, max_chunk_pixels, &plan))
    return refused("block_train_forward_workspace_size: layer%d.%d at B %d x %d x %d, max_chunk_pixels %d is outside the "
                   "plan's range (fewer than 2 values per channel included)",
                   layer, block, B, h, w, max_chunk_pixels);
  return plan.total;
}

extern "C" size_t sfa_block_train_grad_workspace_size(int layer, int block, int B, int h, int w, int max_chunk_pixels) {
  BlockTrainGradPlan plan;
  if (!block_train_grad_plan(layer, block, B, h, w, max_chunk_pixels, &plan))
    return refused("block_train_grad_workspace_size: layer%d.%d at B %d x %d x %d, max_chunk_pixels %d is outside the "
                   "plan's range (fewer than 2 values per channel included)",
                   layer, block, B, h, w, max_chunk_pixels);
  return plan.total;
}

extern "C" int sfa_block_train_chunk_pixels(int layer, int block, int which, int B, int h, int w, int max_chunk_pixels) {
  BlockTrainGradPlan plan;
  if (which < 0 || which > 3 || !block_train_grad_plan(layer, block, B, h, w, max_chunk_pixels, &plan) ||
      (which < 3 && plan.wg[which].taps == 0))
    return refused("block_train_chunk_pixels: item %d of layer%d.%d at B %d x %d x %d, max_chunk_pixels %d does not exist",
                   which, layer, block, B, h, w, max_chunk_pixels);
  return which == 3 ? plan.st.pixels : plan.wg[which].Kc;
}

extern "C" int sfa_block_train_forward(int layer, int block, const float* x, const float* const* params, double eps,
                                       int B, int h, int w, float* z1, float* mid, float* z2, float* zd, float* y,
                                       float* stats, int max_chunk_pixels, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  BlockTrainForwardPlan plan;
  BlockShape sh;
  SFA_CHECK_ARG(B > 0 && h > 0 && w > 0, "block_train_forward: B %d, h %d, w %d must be positive", B, h, w);
  SFA_CHECK_ARG(max_chunk_pixels >= 0, "block_train_forward: max_chunk_pixels %d is negative", max_chunk_pixels);
  SFA_CHECK_ARG(eps >= 0.0 && eps == eps, "block_train_forward: eps must not be negative");
  SFA_CHECK_ARG(block_shape(layer, block, B, h, w, &sh),
                "block_train_forward: layer%d.%d is outside layer1..4, block 0..1, or B %d x %d x %d has a map of 2^31 bytes",
                layer, block, B, h, w);
  SFA_CHECK_ARG(sh.npix_out >= 2,
                "block_train_forward: %d value per channel; training-mode BatchNorm needs more than 1", sh.npix_out);
  SFA_CHECK_ARG(block_train_forward_plan(layer, block, B, h, w, max_chunk_pixels, &plan),
                "block_train_forward: B %d x %d x %d is outside the plan's range", B, h, w);
  const BlockShape& s = plan.s;
  SFA_CHECK_ARG(x && params && z1 && mid && z2 && y && stats && workspace, "block_train_forward: null argument");
  const float* p[9];
  for (int i = 0; i < 9; ++i) p[i] = params[i];
  for (int i = 0; i < 3 * plan.nbn; ++i) SFA_CHECK_ARG(p[i], "block_train_forward: parameter %d is null", i);
  SFA_CHECK_ARG(!s.downsample || zd, "block_train_forward: layer%d.%d has a downsample: zd is needed", layer, block);
  SFA_CHECK_ARG(s.downsample || (!zd && !p[6] && !p[7] && !p[8]),
                "block_train_forward: layer%d.%d has no downsample to take zd or its parameters", layer, block);
  SFA_CHECK_ARG(all_aligned16({x, z1, mid, z2, zd, y, stats, workspace, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}),
                "block_train_forward: every buffer must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "block_train_forward: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  char* ws = reinterpret_cast<char*>(workspace);
  float* wk[3];
  for (int i = 0; i < 3; ++i) wk[i] = reinterpret_cast<float*>(ws + plan.off_wk[i]);
  double* spart = reinterpret_cast<double*>(ws + plan.off_spart);
  float* coef = reinterpret_cast<float*>(ws + plan.off_coef);
  const int C2 = 2 * s.cout;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);

  if (int rc = conv_bn(s, plan.st, x, p[0], p[1], p[2], eps, s.cin, h, w, s.stride, 0, 9, wk[0], z1, spart, stats, coef, st))
    return rc;
  if (int rc = apply(s, z1, coef, nullptr, nullptr, nullptr, mid, st)) return rc;
  if (int rc = conv_bn(s, plan.st, mid, p[3], p[4], p[5], eps, s.cout, s.oh, s.ow, 1, 0, 9, wk[1], z2, spart, stats + C2,
                       coef + C2, st))
    return rc;
  if (s.downsample) {
    if (int rc = conv_bn(s, plan.st, x, p[6], p[7], p[8], eps, s.cin, h, w, s.stride, 4, 1, wk[2], zd, spart,
                         stats + 2 * C2, coef + 2 * C2, st))
      return rc;
    return apply(s, z2, coef + C2, nullptr, zd, coef + 2 * C2, y, st);
  }
  return apply(s, z2, coef + C2, x, nullptr, nullptr, y, st);
}

extern "C" int sfa_block_train_grad(int layer, int block, const float* x, const float* z1, const float* mid,
                                    const float* z2, const float* zd, const float* y, const float* gy,
                                    const float* stats, const float* const* params, double eps, int B, int h, int w,
                                    float* grad_x, float* const* dparams, int max_chunk_pixels, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  BlockTrainGradPlan plan;
  BlockShape sh;
  SFA_CHECK_ARG(B > 0 && h > 0 && w > 0, "block_train_grad: B %d, h %d, w %d must be positive", B, h, w);
  SFA_CHECK_ARG(max_chunk_pixels >= 0, "block_train_grad: max_chunk_pixels %d is negative", max_chunk_pixels);
  SFA_CHECK_ARG(eps >= 0.0 && eps == eps, "block_train_grad: eps must not be negative");
  SFA_CHECK_ARG(block_shape(layer, block, B, h, w, &sh),
                "block_train_grad: layer%d.%d is outside layer1..4, block 0..1, or B %d x %d x %d has a map of 2^31 bytes",
                layer, block, B, h, w);
  SFA_CHECK_ARG(sh.npix_out >= 2, "block_train_grad: %d value per channel; training-mode BatchNorm needs more than 1",
                sh.npix_out);
  SFA_CHECK_ARG(block_train_grad_plan(layer, block, B, h, w, max_chunk_pixels, &plan),
                "block_train_grad: B %d x %d x %d is outside the plan's range", B, h, w);
  const BlockShape& s = plan.s;
  float* dp[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; dparams && i < 9; ++i) dp[i] = dparams[i];
  float *dW1 = dp[0], *dg1 = dp[1], *db1 = dp[2], *dW2 = dp[3], *dg2 = dp[4], *db2 = dp[5], *dWd = dp[6], *dgd = dp[7],
        *dbd = dp[8];
  SFA_CHECK_ARG(x && z1 && mid && z2 && y && gy && stats && params && workspace,
                "block_train_grad: null x, z1, mid, z2, y, gy, stats, params or workspace");
  const float* p[9];
  for (int i = 0; i < 9; ++i) p[i] = params[i];
  SFA_CHECK_ARG(s.downsample || (!dWd && !dgd && !dbd && !zd),
                "block_train_grad: layer%d.%d has no downsample to take zd, dWd, dgammad or dbetad", layer, block);
  SFA_CHECK_ARG(!s.downsample || zd, "block_train_grad: layer%d.%d has a downsample: zd is needed", layer, block);
  // the backward reads the convolution weights and the BatchNorm weights (not the biases)
  for (int i = 0; i < plan.nbn; ++i)
    SFA_CHECK_ARG(p[3 * i] && p[3 * i + 1], "block_train_grad: the weight or the gamma of convolution %d is null", i);
  bool any = grad_x != nullptr;
  for (int i = 0; i < 9; ++i) any = any || dp[i];
  SFA_CHECK_ARG(any, "block_train_grad: no output wanted");
  SFA_CHECK_ARG(all_aligned16({x, z1, mid, z2, zd, y, gy, stats, grad_x, workspace, p[0], p[1], p[3], p[4], p[6], p[7],
                               dp[0], dp[1], dp[2], dp[3], dp[4], dp[5], dp[6], dp[7], dp[8]}),
                "block_train_grad: every buffer must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "block_train_grad: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  char* ws = reinterpret_cast<char*>(workspace);
  float* dZ2 = reinterpret_cast<float*>(ws + plan.off_dz2);
  float* dZd = reinterpret_cast<float*>(ws + plan.off_dzd);
  float* dA = reinterpret_cast<float*>(ws + plan.off_da);
  float* dZ1 = reinterpret_cast<float*>(ws + plan.off_dz1);
  float* Wt1 = reinterpret_cast<float*>(ws + plan.off_wt[0]);
  float* Wt2 = reinterpret_cast<float*>(ws + plan.off_wt[1]);
  float* part = reinterpret_cast<float*>(ws + plan.off_part);
  double* rpart = reinterpret_cast<double*>(ws + plan.off_rpart);
  double* sums = reinterpret_cast<double*>(ws + plan.off_sums);
  const int C2 = 2 * s.cout;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);

  const bool need1 = grad_x || dW1 || dg1 || db1;  // what lies behind conv2
  // BatchNorm 2 and the downsample's: dY = y > 0 ? gy : 0 is never stored
  if (need1 || dW2 || dg2 || db2)
    if (int rc = bn_backward(s, plan.st, gy, y, z2, stats + C2, p[4], eps, rpart, sums, dg2, db2, (need1 || dW2) ? dZ2 : nullptr, st))
      return rc;
  if (s.downsample && (grad_x || dWd || dgd || dbd))
    if (int rc = bn_backward(s, plan.st, gy, y, zd, stats + 2 * C2, p[7], eps, rpart, sums, dgd, dbd,
                             (grad_x || dWd) ? dZd : nullptr, st))
      return rc;
  if (dW2)
    if (int rc = launch_block_wgrad(plan.wg[1], s, dZ2, nullptr, mid, s.oh, s.ow, 1, 0, part, dW2, st)) return rc;
  if (dWd)
    if (int rc = launch_block_wgrad(plan.wg[2], s, dZd, nullptr, x, h, w, s.stride, 4, part, dWd, st)) return rc;
  if (!need1) return SFA_OK;

  // dA = mid > 0 ? dgrad_1(dZ2; W2) : 0, then BatchNorm 1
  if (int rc = relayout(p[3], s.cout, s.cout, 9, nullptr, Wt2, st)) return rc;
  BkDgrad t2;
  memset(&t2, 0, sizeof t2);
  t2.g0 = dZ2, t2.W0 = Wt2, t2.ldw0 = 9 * s.cout, t2.om = mid;
  t2.h = s.oh, t2.w = s.ow, t2.oh = s.oh, t2.ow = s.ow, t2.s = 1, t2.cin = s.cout, t2.cout = s.cout, t2.npix = s.npix_out;
  if (int rc = launch_block_dgrad(t2, dA, st)) return rc;
  if (int rc = bn_backward(s, plan.st, dA, nullptr, z1, stats, p[1], eps, rpart, sums, dg1, db1,
                           (grad_x || dW1) ? dZ1 : nullptr, st))
    return rc;
  if (dW1)
    if (int rc = launch_block_wgrad(plan.wg[0], s, dZ1, nullptr, x, h, w, s.stride, 0, part, dW1, st)) return rc;
  if (!grad_x) return SFA_OK;

  // dx = dgrad_s(dZ1; W1) + the skip
  if (int rc = relayout(p[0], s.cout, s.cin, 9, nullptr, Wt1, st)) return rc;
  BkDgrad t1;
  memset(&t1, 0, sizeof t1);
  t1.g0 = dZ1, t1.W0 = Wt1, t1.ldw0 = 9 * s.cin;
  if (s.downsample)
    t1.g1 = dZd, t1.W1 = p[6], t1.ldw1 = s.cin;  // torch's (Cout, Cin, 1, 1) is [o][c] as it lies
  else
    t1.eg = gy, t1.em = y;
  t1.h = h, t1.w = w, t1.oh = s.oh, t1.ow = s.ow, t1.s = s.stride, t1.cin = s.cin, t1.cout = s.cout, t1.npix = s.npix_in;
  return launch_block_dgrad(t1, grad_x, st);
}
