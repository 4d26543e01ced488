// sfa_model_block_forward / sfa_model_block_grad / sfa_bn_unfold_grad: one BasicBlock of layer1..4
// (models/fpn_resnet.py:42-71) as an operator on a caller's input, BatchNorm folded with its running statistics as
// the handle holds it, and its gradients (gfx950; include/sfa_hip.h has the contract).
//   forward   launch_frame_amax on x, launch_conv (fp16x3, conv1 + shift + ReLU) -> mid, launch_frame_amax on mid,
//             launch_conv (conv2 + shift + skip + ReLU; the downsample as its second K segment) -> y
//   gradient  block_dgrad_kernel   dA = mid > 0 ? dgrad_1(dZ; W2') : 0, dZ = y > 0 ? gy : 0 masked as it is loaded
//             block_wgrad_kernel + the shared fold   dW2' (dZ, mid), dW1' (dA, x), dWd' (dZ, x through the centre tap)
//             the shared bias pair (grad_common.hip)   db2' (dZ), db1' (dA)
//             block_dgrad_kernel   dx = dgrad_s(dA; W1') + the skip: dZ in the epilogue (identity) or the 1x1
//                                  stride-s downsample as a second K segment on the centre tap
//             Only what a wanted output needs is launched.
// Every check is made before the first launch; nothing allocates or synchronises.
#include <cstring>

#include "block_host.h"
#include "block_kernel.h"
#include "conv.h"
#include "dispatch.h"
#include "grad_host.h"

using namespace sfa;

namespace {

int block_level(const char* who, const sfa_model* model, int layer, int block, BlockLevel* bl) {
  SFA_CHECK_ARG(model, "%s: null model", who);
  if (int rc = model_block_level(model, layer, block, bl)) return rc;
  SFA_CHECK_ARG(aligned16(bl->w[0]) && aligned16(bl->w[1]) && bl->K[0] == 9 * bl->cin &&
                    bl->K[1] == 9 * bl->cout + (bl->downsample ? bl->cin : 0),
                "%s: layer%d.%d is not packed as the kernels read it", who, layer, block);
  return SFA_OK;
}

}  // namespace

int sfa::launch_block_wgrad(const BlockWgrad& g, const BlockShape& s, const float* gr, const float* gm, const float* x,
                            int h, int w, int stride, int tap0, float* part, float* dW, hipStream_t st) {
  const BkWgrad t = {gr, gm, x, h, w, s.oh, s.ow, stride, g.cin, g.rows, tap0, g.taps, g.npix, g.Kc};
  const dim3 grid((unsigned)g.chunks, (unsigned)(g.taps * g.cin / kGradTile), (unsigned)(g.rows / kGradTile));
  if (int rc = launch({grid, dim3(256), st}, block_wgrad_kernel, t, part)) return rc;
  return launch_wgrad_fold(part, g.chunks, g.rows, g.cin, g.taps, dW, g.cin, 0, st);
}

int sfa::launch_block_dgrad(const BkDgrad& t, float* out, hipStream_t st) {
  return launch({dim3((unsigned)grad_tiles(t.npix), (unsigned)(t.cin / kGradTile)), dim3(256), st}, block_dgrad_kernel, t,
                out);
}

extern "C" size_t sfa_model_block_forward_workspace_size(const sfa_model* model, int layer, int block, int B, int h,
                                                         int w) {
  BlockLevel bl;
  BlockForwardPlan plan;
  if (block_level("block_forward_workspace_size", model, layer, block, &bl) != SFA_OK) return 0;
  if (!block_forward_plan(layer, block, B, h, w, &plan))
    return refused("block_forward_workspace_size: B %d x %d x %d is outside the plan's range", B, h, w);
  return plan.total;
}

extern "C" int sfa_model_block_forward(const sfa_model* model, int layer, int block, const float* x, int B, int h, int w,
                                       float* mid_out, float* y_out, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  BlockLevel bl;
  BlockForwardPlan plan;
  if (int rc = block_level("block_forward", model, layer, block, &bl)) return rc;
  SFA_CHECK_ARG(B > 0 && h > 0 && w > 0, "block_forward: B %d, h %d, w %d must be positive", B, h, w);
  SFA_CHECK_ARG(block_forward_plan(layer, block, B, h, w, &plan), "block_forward: B %d x %d x %d has a map of 2^31 bytes",
                B, h, w);
  SFA_CHECK_ARG(x && mid_out && y_out && workspace, "block_forward: null argument");
  SFA_CHECK_ARG(all_aligned16({x, mid_out, y_out, workspace}),
                "block_forward: the maps and the workspace must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "block_forward: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  const BlockShape& s = plan.s;
  char* ws = reinterpret_cast<char*>(workspace);
  unsigned* amax_x = reinterpret_cast<unsigned*>(ws + plan.off_amax_x);
  unsigned* amax_mid = reinterpret_cast<unsigned*>(ws + plan.off_amax_mid);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ConvArgs a[2];
  for (int c = 0; c < 2; ++c) {
    memset(&a[c], 0, sizeof a[c]);
    a[c].nseg = 1;
    a[c].Kpad = bl.K[c];
    a[c].w = bl.w[c];
    a[c].wx = bl.wx[c];
    a[c].wh = bl.wh[c];
    a[c].winv = bl.winv[c];
    a[c].bias = bl.b[c];
    a[c].M = s.npix_out;
    a[c].N = s.cout;
    a[c].OH = s.oh;
    a[c].OW = s.ow;
    a[c].relu = 1;
    if (plan.part_floats) {
      a[c].part = reinterpret_cast<float*>(ws + plan.off_part);
      a[c].part_floats = plan.part_floats;
    }
  }
  SFA_CHECK_ARG(make_seg(a[0].seg[0], x, B, h, w, s.cin, 3, s.stride, 1) &&
                    make_seg(a[1].seg[0], mid_out, B, s.oh, s.ow, s.cout, 3, 1, 1),
                "block_forward: a map passes 32-bit byte offsets");
  a[0].amax_in[0] = amax_x;
  a[0].y = mid_out;
  a[1].amax_in[0] = amax_mid;
  a[1].y = y_out;
  if (s.downsample) {
    a[1].nseg = 2;
    a[1].kseg1 = bl.kds;
    make_seg(a[1].seg[1], x, B, h, w, s.cin, 1, s.stride, 0);
    a[1].amax_in[1] = amax_x;
  } else {
    a[1].res = x;
  }
  if (int rc = launch_frame_amax(x, amax_x, B, h * w * s.cin / 4, st)) return rc;
  if (int rc = launch_conv(a[0], EPI_STD, SFA_MATH_FP16X3, st)) return rc;
  if (int rc = launch_frame_amax(mid_out, amax_mid, B, s.oh * s.ow * s.cout / 4, st)) return rc;
  return launch_conv(a[1], EPI_STD, SFA_MATH_FP16X3, st);
}

extern "C" size_t sfa_model_block_grad_workspace_size(const sfa_model* model, int layer, int block, int B, int h, int w,
                                                      int max_chunk_pixels) {
  BlockLevel bl;
  BlockGradPlan plan;
  if (block_level("block_grad_workspace_size", model, layer, block, &bl) != SFA_OK) return 0;
  if (!block_grad_plan(layer, block, B, h, w, max_chunk_pixels, &plan))
    return refused("block_grad_workspace_size: B %d x %d x %d, max_chunk_pixels %d is outside the plan's range", B, h, w,
                   max_chunk_pixels);
  return plan.total;
}

extern "C" int sfa_model_block_grad_chunk_pixels(const sfa_model* model, int layer, int block, int which, int B, int h,
                                                 int w, int max_chunk_pixels) {
  BlockLevel bl;
  BlockGradPlan plan;
  if (block_level("block_grad_chunk_pixels", model, layer, block, &bl) != SFA_OK) return 0;
  if (which < 0 || which > 2 || !block_grad_plan(layer, block, B, h, w, max_chunk_pixels, &plan) ||
      plan.wg[which].taps == 0)
    return refused("block_grad_chunk_pixels: gradient %d of layer%d.%d at B %d x %d x %d, max_chunk_pixels %d does not exist",
                   which, layer, block, B, h, w, max_chunk_pixels);
  return plan.wg[which].Kc;
}

extern "C" int sfa_model_block_grad(const sfa_model* model, int layer, int block, const float* x, const float* mid,
                                    const float* y, const float* gy, int B, int h, int w, float* grad_x,
                                    float* const* dparams, int max_chunk_pixels, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  BlockLevel bl;
  BlockGradPlan plan;
  if (int rc = block_level("block_grad", model, layer, block, &bl)) return rc;
  SFA_CHECK_ARG(B > 0 && h > 0 && w > 0, "block_grad: B %d, h %d, w %d must be positive", B, h, w);
  SFA_CHECK_ARG(max_chunk_pixels >= 0, "block_grad: max_chunk_pixels %d is negative", max_chunk_pixels);
  SFA_CHECK_ARG(block_grad_plan(layer, block, B, h, w, max_chunk_pixels, &plan),
                "block_grad: B %d x %d x %d has a map of 2^31 bytes", B, h, w);
  float* dp[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; dparams && i < 5; ++i) dp[i] = dparams[i];
  float *dW1 = dp[0], *db1 = dp[1], *dW2 = dp[2], *db2 = dp[3], *dWd = dp[4];
  SFA_CHECK_ARG(mid && y && gy && workspace, "block_grad: null mid, y, gy or workspace");
  SFA_CHECK_ARG(bl.downsample || !dWd, "block_grad: layer%d.%d has no downsample to take dWd'", layer, block);
  SFA_CHECK_ARG(grad_x || dW1 || db1 || dW2 || db2 || dWd, "block_grad: no output wanted");
  SFA_CHECK_ARG(x || (!dW1 && !dWd), "block_grad: dW1' and dWd' read x");
  SFA_CHECK_ARG(all_aligned16({x, mid, y, gy, grad_x, dW1, db1, dW2, db2, dWd, workspace}),
                "block_grad: every buffer must be 16-byte aligned");
  SFA_CHECK_ARG(workspace_bytes >= plan.total, "block_grad: workspace of %zu bytes, %zu needed", workspace_bytes,
                plan.total);
  const BlockShape& s = plan.s;
  char* ws = reinterpret_cast<char*>(workspace);
  float* dA = reinterpret_cast<float*>(ws + plan.off_da);
  float* part = reinterpret_cast<float*>(ws + plan.off_part);
  double* bpart = reinterpret_cast<double*>(ws + plan.off_bpart);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);

  // conv2 and the downsample: dZ = y > 0 ? gy : 0 is never stored
  if (db2)
    if (int rc = launch_bias_grad(plan.bs, gy, y, bpart, db2, st)) return rc;
  if (dW2)
    if (int rc = launch_block_wgrad(plan.wg[1], s, gy, y, mid, s.oh, s.ow, 1, 0, part, dW2, st)) return rc;
  if (dWd)
    if (int rc = launch_block_wgrad(plan.wg[2], s, gy, y, x, h, w, s.stride, 4, part, dWd, st)) return rc;
  if (!grad_x && !dW1 && !db1) return SFA_OK;

  // dA = mid > 0 ? dgrad_1(dZ; W2') : 0
  BkDgrad t2;
  memset(&t2, 0, sizeof t2);
  t2.g0 = gy, t2.m0 = y, t2.W0 = bl.w[1], t2.ldw0 = bl.K[1], t2.om = mid;
  t2.h = s.oh, t2.w = s.ow, t2.oh = s.oh, t2.ow = s.ow, t2.s = 1, t2.cin = s.cout, t2.cout = s.cout, t2.npix = s.npix_out;
  if (int rc = launch_block_dgrad(t2, dA, st)) return rc;
  if (db1)
    if (int rc = launch_bias_grad(plan.bs, dA, nullptr, bpart, db1, st)) return rc;
  if (dW1)
    if (int rc = launch_block_wgrad(plan.wg[0], s, dA, nullptr, x, h, w, s.stride, 0, part, dW1, st)) return rc;
  if (!grad_x) return SFA_OK;

  // dx = dgrad_s(dA; W1') + the skip
  BkDgrad t1;
  memset(&t1, 0, sizeof t1);
  t1.g0 = dA, t1.W0 = bl.w[0], t1.ldw0 = bl.K[0];
  if (bl.downsample)
    t1.g1 = gy, t1.m1 = y, t1.W1 = bl.w[1] + bl.kds, t1.ldw1 = bl.K[1];
  else
    t1.eg = gy, t1.em = y;
  t1.h = h, t1.w = w, t1.oh = s.oh, t1.ow = s.ow, t1.s = s.stride, t1.cin = s.cin, t1.cout = s.cout, t1.npix = s.npix_in;
  return launch_block_dgrad(t1, grad_x, st);
}

extern "C" int sfa_bn_unfold_grad(const float* W, const float* gamma, const float* mean, const float* var, double eps,
                                  const float* dWf, const float* dbf, int Cout, int K, float* dW, float* dgamma,
                                  float* dbeta, void* stream) {
  SFA_CHECK_ARG(Cout > 0 && K > 0 && (long long)Cout * K < (1ll << 29), "bn_unfold_grad: Cout %d, K %d out of range", Cout,
                K);
  SFA_CHECK_ARG(eps >= 0.0 && eps == eps, "bn_unfold_grad: eps must not be negative");
  SFA_CHECK_ARG(dW || dgamma || dbeta, "bn_unfold_grad: no output wanted");
  SFA_CHECK_ARG(gamma && var, "bn_unfold_grad: null gamma or var");
  SFA_CHECK_ARG(dWf || (!dW && !dgamma), "bn_unfold_grad: dW and dgamma read dWf");
  SFA_CHECK_ARG(!dgamma || (W && mean), "bn_unfold_grad: dgamma reads W and mean");
  SFA_CHECK_ARG(dbf || (!dgamma && !dbeta), "bn_unfold_grad: dgamma and dbeta read dbf");
  return launch({dim3((unsigned)Cout), dim3(256), reinterpret_cast<hipStream_t>(stream)}, bn_unfold_kernel, W, gamma, mean,
                var, eps, (dW || dgamma) ? dWf : nullptr, dbf, K, dW, dgamma, dbeta);
}
