// sfa_model_heads_grad: the parameter gradients of one KFPN level's detection heads (gfx950).  What
// total_loss.backward() leaves at fpn{level}_{head}.0.weight / .0.bias / .2.weight / .2.bias
// (models/fpn_resnet.py:135-143, train.py:190-247) given d total / d (the level's head outputs), which
// sfa_kfpn_combine_grad writes.  Stages, all on the caller's stream (include/sfa_hip.h has the contract):
//   1. hidden recompute   Hd = ReLU(conv3x3(x; W1) + b1) for every head of the level, always in fp16x3 whatever the
//                         model's mode is: launch_conv with the standard epilogue.  Its fp16x3 kernels take 64 or a
//                         multiple of 128 columns, so the 64 * heads columns run as one launch over the first
//                         heads / 2 * 128 and one over the last 64 (odd head counts), each on a copy of the packed
//                         fp16 terms cut at that column (heads_terms_cut_kernel, into the workspace: the packed
//                         layout is untouched) and on the frames' own max |x| (heads_amax_kernel: x may be any
//                         caller buffer, so no producer recorded it)
//   2. heads_dhidden_kernel + heads_dhidden_fold_kernel   dA, dW2, db2, db1
//   3. heads_wgrad_kernel   the hot path: per K-chunk partial dW1 tiles on f32 MFMA
//   4. heads_wgrad_fold_kernel   the chunks added in chunk order in float64
// sfa_model_heads_input_grad: heads_dgrad_kernel on the dA that stage 2 leaves, one launch.
// sfa_model_heads_forward: stage 1 (the same helper, so the same Hd bits), then heads_out_kernel.
#include <cstring>

#include "conv.h"
#include "dispatch.h"
#include "grad_host.h"
#include "heads_grad_kernel.h"

using namespace sfa;

int sfa::launch_frame_amax(const float* x, unsigned* amax, int B, int n4, hipStream_t st) {
  return launch({dim3(8, (unsigned)B), dim3(256), st}, heads_amax_kernel, reinterpret_cast<const float4*>(x), amax, n4);
}

namespace {

// The checks the two entries share: the level's parameters and the plan.
int heads_grad_setup(const char* who, const sfa_model* model, int level, int B, int h, int w, int max_chunk_pixels,
                     HeadsLevel* hl, HeadsGradPlan* plan) {
  SFA_CHECK_ARG(model, "%s: null model", who);
  if (int rc = model_heads_level(model, level, hl)) return rc;
  SFA_CHECK_ARG(B > 0 && h > 0 && w > 0, "%s: B %d, h %d, w %d must be positive", who, B, h, w);
  SFA_CHECK_ARG(max_chunk_pixels >= 0, "%s: max_chunk_pixels %d is negative", who, max_chunk_pixels);
  SFA_CHECK_ARG(heads_grad_plan(B, h, w, hl->Cin, hl->num_heads, max_chunk_pixels, plan),
                "%s: B %d x %d x %d with %d / %d channels passes 32-bit byte offsets", who, B, h, w, hl->Cin,
                64 * hl->num_heads);
  return SFA_OK;
}

// Stage 1 of both entries: Hd = ReLU(conv3x3(x; W1) + b1) in fp16x3 into hidden ([pixels][Na] then [pixels][Nb]):
// the level's terms cut at the column split, the frames' max |x|, one convolution per part.
int heads_hidden_stage(const HeadsLevel& hl, const float* x, int B, int h, int w, int Na, int Nb, float* hidden,
                       uint16_t* terms, unsigned* amax, hipStream_t st) {
  const int Cin = hl.Cin, M = Na + Nb, K = 9 * Cin, npix = B * h * w;
  float* hidden_b = hidden + (size_t)npix * Na;
  if (int rc = launch({dim3((unsigned)ceil_div(M * K, 256)), dim3(256), st}, heads_terms_cut_kernel,
                      reinterpret_cast<const uint32_t*>(hl.wh), reinterpret_cast<uint32_t*>(terms),
                      reinterpret_cast<uint32_t*>(terms + (size_t)2 * Na * K), M, Na, K / 2))
    return rc;
  if (int rc = launch_frame_amax(x, amax, B, h * w * Cin / 4, st)) return rc;
  for (int part_i = 0; part_i < 2; ++part_i) {
    const int n0 = part_i ? Na : 0, N = part_i ? Nb : Na;
    if (N == 0) continue;
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.nseg = 1;
    SFA_CHECK_ARG(make_seg(a.seg[0], x, B, h, w, Cin, 3, 1, 1), "heads_grad: x passes 32-bit byte offsets");
    a.Kpad = K;
    a.w = hl.w3 + (size_t)n0 * K;
    a.wh = terms + (size_t)2 * n0 * K;
    a.winv = hl.winv + n0;
    a.amax_in[0] = amax;
    a.bias = hl.b3 + n0;
    a.y = part_i ? hidden_b : hidden;
    a.M = npix;
    a.N = N;
    a.OH = h;
    a.OW = w;
    a.relu = 1;
    if (int rc = launch_conv(a, EPI_STD, SFA_MATH_FP16X3, st)) return rc;
  }
  return SFA_OK;
}

}  // namespace

extern "C" size_t sfa_model_heads_grad_workspace_size(const sfa_model* model, int level, int B, int h, int w,
                                                      int max_chunk_pixels) {
  HeadsLevel hl;
  HeadsGradPlan plan;
  if (heads_grad_setup("heads_grad_workspace_size", model, level, B, h, w, max_chunk_pixels, &hl, &plan) != SFA_OK)
    return 0;
  return plan.total;
}

extern "C" int sfa_model_heads_grad_chunk_pixels(const sfa_model* model, int level, int B, int h, int w,
                                                 int max_chunk_pixels) {
  HeadsLevel hl;
  HeadsGradPlan plan;
  if (heads_grad_setup("heads_grad_chunk_pixels", model, level, B, h, w, max_chunk_pixels, &hl, &plan) != SFA_OK)
    return 0;
  return plan.Kc;
}

extern "C" int sfa_model_heads_grad(const sfa_model* model, int level, const float* x, int B, int h, int w,
                                    const float* const* grad_levels, float* const* grad_w1, float* const* grad_b1,
                                    float* const* grad_w2, float* const* grad_b2, float* hidden_out,
                                    float* dhidden_out, int max_chunk_pixels, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  HeadsLevel hl;
  HeadsGradPlan plan;
  if (int rc = heads_grad_setup("heads_grad", model, level, B, h, w, max_chunk_pixels, &hl, &plan)) return rc;
  SFA_CHECK_ARG(x && grad_levels && grad_w1 && grad_b1 && grad_w2 && grad_b2 && workspace,
                "heads_grad: null argument");
  HgHeads t;
  memset(&t, 0, sizeof t);
  t.num_heads = hl.num_heads;
  for (int j = 0; j < hl.num_heads; ++j) {
    SFA_CHECK_ARG(grad_levels[j] && grad_w1[j] && grad_b1[j] && grad_w2[j] && grad_b2[j],
                  "heads_grad: null pointer for head %d", j);
    t.g[j] = grad_levels[j];
    t.gw1[j] = grad_w1[j];
    t.gb1[j] = grad_b1[j];
    t.gw2[j] = grad_w2[j];
    t.gb2[j] = grad_b2[j];
    t.ch[j] = hl.ch[j];
  }
  SFA_CHECK_ARG(all_aligned16({x, workspace, hidden_out, dhidden_out}),
                "heads_grad: x, workspace, hidden_out and dhidden_out must be 16-byte aligned");
  if (workspace_bytes < plan.total) {
    set_error("heads_grad: workspace of %zu bytes, %zu needed", workspace_bytes, plan.total);
    return SFA_E_WORKSPACE;
  }
  char* ws = reinterpret_cast<char*>(workspace);
  float* hidden = reinterpret_cast<float*>(ws + plan.off_hidden);  // two column parts; hidden_out gets the joined copy
  float* dhidden = dhidden_out ? dhidden_out : reinterpret_cast<float*>(ws + plan.off_dhidden);
  float* part = reinterpret_cast<float*>(ws + plan.off_part);
  double* dpart = reinterpret_cast<double*>(ws + plan.off_dpart);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int M = plan.M, Cin = plan.Cin, npix = B * h * w;

  // 1. Hd in fp16x3
  float* hidden_b = hidden + (size_t)npix * plan.Na;
  if (int rc = heads_hidden_stage(hl, x, B, h, w, plan.Na, plan.Nb, hidden,
                                  reinterpret_cast<uint16_t*>(ws + plan.off_terms),
                                  reinterpret_cast<unsigned*>(ws + plan.off_amax), st))
    return rc;
  const int Na = plan.Na;

  // 2. dA and the float64 sums
  if (int rc = launch({dim3((unsigned)plan.dh_blocks), dim3((unsigned)M), st}, heads_dhidden_kernel, t, hidden, hidden_b,
                      Na, hidden_out, hl.w1, dhidden, dpart, npix, h * w, plan.dh_pixels, M))
    return rc;
  if (int rc = launch({dim3((unsigned)ceil_div(plan.dh_slots, 256)), dim3(256), st}, heads_dhidden_fold_kernel, t, dpart,
                      plan.dh_blocks, M))
    return rc;

  // 3. + 4. dW1
  const dim3 grid((unsigned)plan.num_chunks, (unsigned)(Cin / kHgTile), (unsigned)(M / kHgTile));
  if (int rc = launch({grid, dim3(256), st}, heads_wgrad_kernel, dhidden, x, part, h, w, Cin, M, plan.rows_per_chunk,
                      plan.chunks_per_frame))
    return rc;
  return launch({dim3((unsigned)ceil_div(M * Cin * 9, 256)), dim3(256), st}, heads_wgrad_fold_kernel, t, part,
                plan.num_chunks, Cin, M);
}

extern "C" int sfa_heads_dgrad_pixel_tile(void) { return kHgDgPix; }

extern "C" int sfa_model_heads_input_grad(const sfa_model* model, int level, const float* dhidden, int B, int h, int w,
                                          float* grad_x, void* stream) {
  HeadsLevel hl;
  HeadsGradPlan plan;
  if (int rc = heads_grad_setup("heads_input_grad", model, level, B, h, w, 0, &hl, &plan)) return rc;
  HeadsDgradPlan dg;
  SFA_CHECK_ARG(heads_dgrad_plan(B, h, w, hl.Cin, hl.num_heads, &dg), "heads_input_grad: B %d x %d x %d has too many tiles",
                B, h, w);
  SFA_CHECK_ARG(dhidden && grad_x, "heads_input_grad: null argument");
  SFA_CHECK_ARG(all_aligned16({dhidden, grad_x, hl.w3}),
                "heads_input_grad: dhidden, grad_x and the model's weights must be 16-byte aligned");
  return launch({dim3((unsigned)dg.blocks), dim3(256), reinterpret_cast<hipStream_t>(stream)}, heads_dgrad_kernel, dhidden,
                hl.w3, grad_x, h, w, hl.Cin, plan.M, dg.tiles_per_row, dg.chan_tiles);
}

extern "C" size_t sfa_model_heads_forward_workspace_size(const sfa_model* model, int level, int B, int h, int w) {
  HeadsLevel hl;
  HeadsGradPlan plan;
  HeadsForwardPlan fp;
  if (heads_grad_setup("heads_forward_workspace_size", model, level, B, h, w, 0, &hl, &plan) != SFA_OK) return 0;
  return heads_forward_plan(B, h, w, hl.Cin, hl.num_heads, &fp) ? fp.total : 0;
}

extern "C" int sfa_model_heads_forward(const sfa_model* model, int level, const float* x, int B, int h, int w,
                                       float* const* y_levels, float* hidden_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  HeadsLevel hl;
  HeadsGradPlan plan;
  HeadsForwardPlan fp;
  if (int rc = heads_grad_setup("heads_forward", model, level, B, h, w, 0, &hl, &plan)) return rc;
  SFA_CHECK_ARG(heads_forward_plan(B, h, w, hl.Cin, hl.num_heads, &fp), "heads_forward: no plan");
  SFA_CHECK_ARG(x && y_levels && workspace, "heads_forward: null argument");
  HoHeads t;
  memset(&t, 0, sizeof t);
  t.num_heads = hl.num_heads;
  for (int j = 0; j < hl.num_heads; ++j) {
    SFA_CHECK_ARG(y_levels[j], "heads_forward: null pointer for head %d", j);
    t.y[j] = y_levels[j];
    t.ch[j] = hl.ch[j];
  }
  SFA_CHECK_ARG(all_aligned16({x, workspace, hidden_out}),
                "heads_forward: x, workspace and hidden_out must be 16-byte aligned");
  if (workspace_bytes < fp.total) {
    set_error("heads_forward: workspace of %zu bytes, %zu needed", workspace_bytes, fp.total);
    return SFA_E_WORKSPACE;
  }
  char* ws = reinterpret_cast<char*>(workspace);
  float* hidden = reinterpret_cast<float*>(ws + fp.off_hidden);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int npix = B * h * w;
  if (int rc = heads_hidden_stage(hl, x, B, h, w, fp.Na, fp.Nb, hidden, reinterpret_cast<uint16_t*>(ws + fp.off_terms),
                                  reinterpret_cast<unsigned*>(ws + fp.off_amax), st))
    return rc;
  return launch({dim3((unsigned)ceil_div(npix * hl.num_heads * 4, 256)), dim3(256), st}, heads_out_kernel, t, hidden,
                hidden + (size_t)npix * fp.Na, fp.Na, fp.M, hidden_out, hl.w1, hl.b1, npix, h * w);
}
