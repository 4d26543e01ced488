/*
 * sfa_hip.h — C ABI of the MI355X (gfx950) hot path of the SFA3D-style
 * FPN-ResNet-18 LiDAR detector: BEV voxelisation -> KFPN forward -> decode
 * (and of its plain ResNet-18 sibling, arch "resnet_18": sfa_arch_ex).
 *
 * Plain C: pointers, sizes and status codes only; no torch / C++ types.
 * Every entry point that touches the device takes the caller's hipStream_t
 * (passed as void*), never allocates, never synchronises, and is re-entrant
 * per stream; all buffers (including scratch/workspace) are owned by the
 * caller.  Return value: SFA_OK (0) or a negative SFA_E_* code, with a
 * human-readable reason in sfa_last_error_string() (thread-local).
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to the reference repository root).
 */
#ifndef SFA_HIP_H_
#define SFA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFA_ABI_VERSION 2  /* 2: sfa_bev_voxelize takes scratch_bytes */

enum sfa_status {
  SFA_OK = 0,
  SFA_E_INVALID = -1,   /* bad argument / shape */
  SFA_E_UNSUPPORTED = -2, /* configuration the kernels do not cover */
  SFA_E_HIP = -3,       /* a HIP runtime call failed */
  SFA_E_WORKSPACE = -4  /* workspace / scratch too small */
};

int sfa_abi_version(void);
const char* sfa_last_error_string(void);

/* ------------------------------------------------------------------ BEV --
 * Replaces data_process/kitti_data_utils.py:228-251 get_filtered_lidar followed
 * by data_process/kitti_bev_utils.py:22-55 makeBEVMap, for a batch of frames.
 *
 * points          device, float32 [total_points][4] = x, y, z, intensity (raw,
 *                 unfiltered; the kernel applies the inclusive boundary test)
 * frame_offsets   HOST, int64 [batch + 1]; frame b = points[off[b], off[b+1])
 * batch           1 .. SFA_BEV_MAX_BATCH
 * boundary        HOST, double [6] = minX, maxX, minY, maxY, minZ, maxZ
 *                 (config/kitti_config.py:23-30)
 * flags           SFA_BEV_RAW: raw sweep in, the get_filtered_lidar box test and
 *                 z -= minZ are fused in (the fast path);
 *                 SFA_BEV_PREFILTERED: points already went through
 *                 get_filtered_lidar (makeBEVMap's own contract); no box test.
 * out_layout      SFA_BEV_NCHW3_F32  (B, 3, 608, 608) float32  (== .float() of the
 *                                    reference's float64 map, test.py:124)
 *                 SFA_BEV_NCHW3_F64  (B, 3, 608, 608) float64  (reference dtype)
 *                 SFA_BEV_NHWC4_F32  (B, 608, 608, 4) float32, channel 3 = 0
 *                                    (the model's input layout; no transpose)
 *                 | SFA_BEV_FLIP_HW: the map is written flipped in both spatial
 *                 dims (torch.flip(bev, [1, 2]), utils/demo_utils.py:110-111 — the
 *                 back view of demo_2_sides.py with boundary_back)
 * scratch         device, scratch_bytes >= sfa_bev_scratch_size(batch) bytes (else
 *                 SFA_E_WORKSPACE), ZERO on first use; every call leaves it zeroed again
 *                 except the record regions, which are written before they are read.  The
 *                 layout is set by the capacity (the largest batch scratch_bytes holds), not
 *                 by the call's batch, so calls of any batch may share one scratch.
 * Kernels: one pass bins every 1024 points of a frame by 4-row strips of the map into
 * the pass block's own record region + a per-strip table, then one block per (frame, strip)
 * reduces its runs in LDS, while the batch's regions fit the scratch (~277 k points per
 * frame; SFA_BEV_STRIP8: 8-row strips); SFA_BEV_FORCE_BINNED: round 2's count / scan / bin / strip form; otherwise (or with
 * SFA_BEV_FORCE_ATOMIC) device-scope atomics on a per-cell scratch.  All give the same bits.
 */
#define SFA_BEV_MAX_BATCH 64
enum sfa_bev_layout { SFA_BEV_NCHW3_F32 = 0, SFA_BEV_NCHW3_F64 = 1, SFA_BEV_NHWC4_F32 = 2 };
enum sfa_bev_flags {
  SFA_BEV_RAW = 0, SFA_BEV_PREFILTERED = 1, SFA_BEV_FLIP_HW = 2, SFA_BEV_FORCE_ATOMIC = 4,
  SFA_BEV_FORCE_BINNED = 8,  /* round 2's count / scan / bin / strip kernels (A/B) */
  SFA_BEV_STRIP8 = 16        /* the one-pass path with 8-row strips (round 3a; A/B) */
};

size_t sfa_bev_scratch_size(int batch);
int sfa_bev_voxelize(const float* points, const int64_t* frame_offsets, int batch,
                     const double* boundary, int flags, int out_layout, void* out, void* scratch,
                     size_t scratch_bytes, void* stream);

/* ------------------------------------------------------- Argoverse BEV --
 * Replaces argoverse_test2.py:198-257 makeBVFeature(points, discretization, boundary) (the same
 * function as argoverse_test.py:199-254), for a batch of sweeps, bit for bit on float32 points:
 * closed box test on all six sides; row = clip(trunc((maxX - x) / d), 0, H - 1), col =
 * clip(trunc((y - minY) / d), 0, W - 1) in f32; per cell the INDEPENDENT maxima of max(0, z - minZ)
 * and max(0, intensity) and the point count; channels (density, height, intensity) =
 * (min(n / 10, 1), h / f32(maxZ - minZ), i / the frame's largest cell intensity when that is > 0).
 * A frame with no point inside the box gives zeros.
 *
 * sfa_argo_bev_shape (HOST only, :224-225): H = int((maxX - minX) / d), W = int((maxY - minY) / d)
 * in double.  SFA_E_INVALID for a null pointer, a non-finite value, d <= 0 or an inverted boundary
 * (minX >= maxX, minY >= maxY, minZ > maxZ); SFA_E_UNSUPPORTED when H or W is outside
 * [1, SFA_ARGO_BEV_MAX_DIM] (608 x 608 and the scripts' 800 x 800 are inside).
 *
 * sfa_argo_bev_voxelize
 * points          device, float32 [total_points][point_stride]; columns 0..3 = x, y, z, intensity
 * point_stride    floats per point: 3 (no intensity column: every point has intensity 0.5, :201-203)
 *                 or >= 4 (:204-205); 0, 1, 2 and negative values are SFA_E_INVALID (the reference
 *                 raises ValueError).  Stride 4 with 16-B aligned points is read as float4.
 * frame_offsets   HOST, int64 [batch + 1], in points; frame b = points[off[b], off[b+1])
 * batch           1 .. SFA_BEV_MAX_BATCH (64)
 * boundary        HOST, double [6] = minX, maxX, minY, maxY, minZ, maxZ; discretization: metres per cell
 * out_layout      SFA_BEV_NCHW3_F32 (B, 3, H, W) float32, the reference's map, or SFA_BEV_NHWC4_F32
 *                 (B, H, W, 4) float32 with channel 3 = 0 (SFA_IN_NHWC4, the model's input layout);
 *                 SFA_BEV_NCHW3_F64 is SFA_E_INVALID (the reference returns float32);
 *                 | SFA_ARGO_BEV_FORCE_ATOMIC: the atomic path (A/B, the equivalence test).  out: 16-B aligned.
 * scratch         device, 16-B aligned, scratch_bytes >= sfa_argo_bev_scratch_size(batch, H, W) (else
 *                 SFA_E_WORKSPACE; the size is 0 for a batch or map out of range), ZERO on first use.
 *                 Its first half holds the frames' intensity maxima (one word each, raised by one
 *                 atomicMax per block of the binning pass, read by the pass that writes the map,
 *                 zeroed again by the call's last launch) and the atomic path's 12 B per cell; every
 *                 call leaves that half zeroed.  The second half holds the record path's regions and
 *                 table, written before they are read and left dirty.  The halves are split by
 *                 scratch_bytes alone, so calls of any batch and map size it holds may share one scratch.
 * Kernels: the KITTI voxeliser's one-pass form — every 1024 points of a frame binned by strips of the
 * map (<= 4096 cells) into the pass block's own record region (10 B per point) + a per-strip table,
 * then one block per (frame, strip) reducing its runs in LDS — while the batch's regions fit the second
 * half (800 x 800: ~720 k points per frame of the batch on average, at most 1 Mi in one frame);
 * otherwise device-scope atomics on the per-cell scratch.  Both give the same bits; nothing is
 * truncated: a frame of >= 2^32 - 1 points is SFA_E_UNSUPPORTED.  All argument errors are
 * reported before any device call. */
#define SFA_ARGO_BEV_MAX_DIM 2048
#define SFA_ARGO_BEV_FORCE_ATOMIC 0x100
int sfa_argo_bev_shape(const double* boundary, double discretization, int* H, int* W);
size_t sfa_argo_bev_scratch_size(int batch, int H, int W);
int sfa_argo_bev_voxelize(const float* points, int point_stride, const int64_t* frame_offsets, int batch,
                          const double* boundary, double discretization, int out_layout, void* out,
                          void* scratch, size_t scratch_bytes, void* stream);

/* Replaces data_process/kitti_data_utils.py:228-251 get_filtered_lidar (labels=None):
 * order-preserving compaction of the points inside the inclusive box, with
 * z <- z - minZ.  points/out device float32 [n][4]; out must hold n points;
 * *out_count (DEVICE int64) receives the kept count.  scratch: device,
 * sfa_filter_scratch_size(n) bytes. */
size_t sfa_filter_scratch_size(int64_t n_points);
int sfa_filter_points(const float* points, int64_t n_points, const double* boundary, float* out,
                      int64_t* out_count, void* scratch, size_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------- model --
 * Replaces models/model_utils.py:25-43 create_model -> models/fpn_resnet.py
 * get_pose_net(18, heads, 64) (:296-301) and PoseResNet.forward (:169-246).
 *
 * Architecture descriptor: resnet depth (18 only), head_conv (64 only) and the
 * heads in FORWARD order (the `heads` dict insertion order, fpn_resnet.py:220);
 * the state_dict registers them in sorted() order (fpn_resnet.py:135).
 */
#define SFA_MAX_HEADS 8
typedef struct sfa_arch {
  int num_layers;                 /* 18 */
  int head_conv;                  /* 64 */
  int num_heads;                  /* 1 .. SFA_MAX_HEADS */
  int head_channels[SFA_MAX_HEADS]; /* 1 .. 4 each, forward order */
  char head_names[SFA_MAX_HEADS][32];
} sfa_arch;

/* Reference state_dict layout (186 entries for fpn_resnet_18 with 5 heads), in
 * nn.Module registration order.  shape is padded with 0s; ndim 0 = scalar. */
int sfa_state_count(const sfa_arch* arch);
int sfa_state_entry(const sfa_arch* arch, int index, char* name, int name_len, int64_t* shape4,
                    int* ndim);

/* Pack weights (host -> host): `state` = the float32 values of every
 * state_dict entry except *.num_batches_tracked, concatenated in
 * sfa_state_entry order.  BatchNorm (eps 1e-5) is folded into the preceding
 * convolution; conv weights are re-laid out OHWI / K-concatenated for the
 * implicit-GEMM kernels, each also stored as three bf16 terms for SFA_MATH_BF16X6 and,
 * scaled per output channel by a power of two, as two fp16 terms for SFA_MATH_FP16X3.
 * `packed` must hold sfa_packed_floats(arch) floats. */
size_t sfa_state_floats(const sfa_arch* arch);
size_t sfa_packed_floats(const sfa_arch* arch);
int sfa_pack_weights(const sfa_arch* arch, const float* state, size_t state_floats, float* packed);

/* Second detector family (models/model_utils.py:34-37 -> models/resnet.py get_pose_net(18, heads, 64),
 * PoseResNet.forward :219-234): arch "resnet_18", the plain CenterNet-style model — the same stem and
 * residual layers, then three ConvTranspose2d(k=4, s=2, p=1, bias=False) + BatchNorm + ReLU layers
 * (512 -> 256 -> 256 -> 256, H/32 -> H/4) and the heads (conv3x3 -> ReLU -> conv1x1) on that one
 * 256-channel map; no FPN, no apply_kfpn.  sfa_arch cannot grow (the ABI version is pinned), so the family
 * is named beside it: the sfa_arch entry points above are the SFA_BACKBONE_KFPN case of the _ex ones,
 * with identical results.  reserved must be zero; a nonzero word or an unknown backbone is
 * SFA_E_INVALID (-1 / 0 from the count / size entry points); depths other than 18 stay refused.
 * State layout of SFA_BACKBONE_DECONV (resnet.py registration order): the stem and layers as above,
 * deconv_layers.{0,3,6}.weight (512|256, 256, 4, 4) — (Cin, Cout, kh, kw), not OIHW — each followed by
 * its BatchNorm deconv_layers.{1,4,7}.*, then the heads in sorted() order under their plain names:
 * <head>.0.weight (64, 256, 3, 3), .0.bias, .2.weight, .2.bias.  Packed: each transposed conv as the
 * four 2 x 2 phase matrices [256][4 Cin] of its output parities (BN scale folded in, BN shift as the
 * bias), in f32 and as the two fp16 terms of SFA_MATH_FP16X3 (no bf16 terms). */
enum sfa_backbone { SFA_BACKBONE_KFPN = 0, SFA_BACKBONE_DECONV = 1 };
typedef struct sfa_arch_ex {
  sfa_arch base;
  int backbone;     /* sfa_backbone */
  int reserved[7];  /* zero */
} sfa_arch_ex;
int sfa_state_count_ex(const sfa_arch_ex* arch);
int sfa_state_entry_ex(const sfa_arch_ex* arch, int index, char* name, int name_len, int64_t* shape4,
                       int* ndim);
size_t sfa_state_floats_ex(const sfa_arch_ex* arch);
size_t sfa_packed_floats_ex(const sfa_arch_ex* arch);
int sfa_pack_weights_ex(const sfa_arch_ex* arch, const float* state, size_t state_floats, float* packed);

/* Pack weights (device -> device): the bytes sfa_pack_weights(_ex) writes for the same state, written by
 * kernels on `stream` from the state tensors where they live.  state[i] = the device pointer of entry i in
 * sfa_state_entry(_ex) order (float32, contiguous), NULL exactly at the *.num_batches_tracked entries;
 * count = sfa_state_count(_ex); packed_device = sfa_packed_floats(_ex) floats of device memory, 16-byte
 * aligned, every byte of which is written (padding and alignment gaps as zeros).  Stream-ordered: no host
 * synchronisation, no allocation, no memset; capturable in a HIP graph, which then holds the pointers.  A null
 * or non-null pointer in the wrong slot, a wrong count, a pointer that is not memory of the current device and a
 * misaligned packed_device are SFA_E_INVALID, and nothing is written.  A model handle over `packed_device`
 * needs sfa_model_refresh_weight_images on the same stream afterwards (below). */
int sfa_pack_weights_device(const sfa_arch* arch, const float* const* state, int count, float* packed_device,
                            void* stream);
int sfa_pack_weights_device_ex(const sfa_arch_ex* arch, const float* const* state, int count, float* packed_device,
                               void* stream);

/* A model handle references a device copy of the packed weights (caller-owned,
 * must outlive the handle).  No device memory is allocated.  The handle owns side
 * streams + events on the device current at creation: a forward on a stream of that
 * device runs the level-0 detection heads on a side stream (overlapping the rest of the FPN)
 * and the level-2 heads beside the level-1 heads, forked/joined by events, so HIP-graph capture of the
 * caller's stream records every branch; on another device everything stays on the caller's
 * stream. */
typedef struct sfa_model sfa_model;
int sfa_model_create(const sfa_arch* arch, const float* packed_device, sfa_model** out);
/* The same for either family.  A SFA_BACKBONE_DECONV model has no parallel branch: it creates no side
 * streams, every launch of its forward is on the caller's stream and sfa_model_set_side_streams is a
 * no-op on it (returns SFA_OK). */
int sfa_model_create_ex(const sfa_arch_ex* arch, const float* packed_device, sfa_model** out);
/* A second handle over the SAME packed weights as `model` (its own side stream and events, the same
 * family, math left at the default, options seeded as at create), sharing `model`'s derived weight
 * images (below) instead of building them again.  Either handle may be destroyed first. */
int sfa_model_create_twin(const sfa_model* model, sfa_model** out);
void sfa_model_destroy(sfa_model* model);

/* Derived weight images.  For the fp16x3 kernels that stage W by LDS-DMA, create builds a second device
 * buffer owned by the handle: the fp16 terms of those convs permuted once into the byte order of the
 * kernel's LDS tiles, K-tile by K-tile (today: the detection heads' 3x3 convs, ~5.2 MB for the default
 * heads).  The packed buffer itself is never changed.  The images are built at sfa_model_create(_ex)
 * from the packed weights as they are at that moment (on the null stream, waited for), so the upload of
 * `packed_device` must be complete by then; they are built only when `packed_device` is device memory
 * of the current device covering sfa_packed_floats floats (otherwise the handle keeps the kernels that
 * read the packed terms directly, with the same results).  The packed buffer stays the caller's: after
 * ANY later change of its contents, call sfa_model_refresh_weight_images(model, stream) before the next
 * forward; it rebuilds every image on `stream` (stream-ordered, no allocation, capturable) for this
 * handle and its twins.  A stale image cannot be detected.  A caller that updates weights in place and
 * cannot make that call turns the images off with SFA_OPT_W_IMAGES = 0.  (The Python model makes that call after
 * every sfa_pack_weights_device into the buffer of a handle it keeps, optimiser steps included.) */
int sfa_model_refresh_weight_images(sfa_model* model, void* stream);
/* Bytes of device memory the handle's derived weight images of the detection heads take (shared with its
 * twins); 0: it has none. */
size_t sfa_model_weight_image_bytes(const sfa_model* model);
/* The residual layers' 3x3 / stride-1 convs (all of layer1, block 1 of layers 2 - 4) have derived weight images
 * too, in a second device buffer under the same rules (built at create, shared with twins, rebuilt by
 * sfa_model_refresh_weight_images, read only when SFA_OPT_W_IMAGES and SFA_OPT_BODY_W_IMAGES are both 1).
 * Its bytes (the size of those convs' fp16 terms again, ~25 MB); 0: the handle has none. */
size_t sfa_model_body_weight_image_bytes(const sfa_model* model);

/* Side streams on (1, the default; env SFA_SIDE_STREAMS=0 at create time turns them off) or
 * off (0: every launch of the forward on the caller's stream).  Off destroys them (after their
 * last forward has finished), on creates them on the current device.  Every stream of a
 * process takes one of HIP's hardware queues (4 by default), so a caller running several
 * forwards in flight beside a copy stream turns them off (the KITTI .bin stream workload:
 * profiles/r02b_stream_side_streams.txt).  Not concurrently with a forward of this model.
 * No reference counterpart (measurement / scheduling). */
int sfa_model_set_side_streams(sfa_model* model, int on);

/* Arithmetic of the convolutions (all results are f32; every mode meets the parity
 * bar):
 *   SFA_MATH_FP16X3 (default) — operands scaled by powers of two (weights per output channel at
 *     pack time, activations per tensor and frame from the max |x| their producer records) and
 *     split into two fp16 terms (22 significand bits), the three significant products on
 *     fp16 MFMA with f32 accumulation: half the MFMA work of BF16X6 at the same accuracy
 *     class (max rel. logit error vs the reference ~3e-6); the scales never overflow fp16
 *     (scaled |x| < 2^14), and each frame is scaled by its own maxima (batch-invariant);
 *   SFA_MATH_BF16X6 — every f32 operand split into three bf16 terms, the six significant
 *     products on bf16 MFMA with f32 accumulation (full f32 exponent range, no scaling);
 *   SFA_MATH_F32 — v_mfma_f32_32x32x2_f32 (exact f32 FMA chains).
 * Opt-in reduced precision (does NOT meet the parity bar):
 *   SFA_MATH_FP16 — operands scaled exactly as in FP16X3 (weights per output channel at pack time,
 *     activations per tensor and frame), each rounded ONCE to fp16 (round-to-nearest-even: the high
 *     term of the FP16X3 split, the low terms are neither formed nor read), one product per MAC on
 *     v_mfma_f32_16x16x32_f16 with f32 accumulation: a third of FP16X3's matrix work in the residual
 *     layers' convolutions and the detection heads (95 % of the FLOPs).  Results and every tensor in
 *     device memory stay f32; the epilogues (scale-back, bias, residual, ReLU, the heads' 1x1 conv)
 *     are the f32 ones.  The stem and the FPN 1x1 convolutions (VALU / memory bound, 5.5 % of the
 *     FLOPs) run FP16X3 in this mode, which is strictly more accurate, and so does any shape
 *     without a one-product kernel (e.g. a head count other than 5): the mode never fails where
 *     FP16X3 succeeds.  Error of the arithmetic against the reference (max |d| / max(1, |ref|) over
 *     the heads, f64-accumulating CPU restatement, profiles/fp16_error_budget.json): 3.8e-3 / 4.0e-3
 *     on the two small fixture cases, 2.6e-3 on the 608 x 608 frame, 4.6e-3 on the 16 bench frames
 *     (FP16X3: <= 9.3e-6), 795 of the bench batch's 800 reference detections found at the same
 *     pixel with the same class; the GPU kernels are held to 2x of these (tests/test_gpu_math_fp16.py).
 * SFA_BACKBONE_DECONV models run SFA_MATH_FP16X3 only: the transposed convolutions have an fp16x3 kernel
 * alone, so sfa_model_set_math(SFA_MATH_F32 / SFA_MATH_BF16X6) returns SFA_E_UNSUPPORTED on them, and so
 * does SFA_MATH_FP16 until its logit error on this architecture has a budget (the CPU restatement of the
 * one-product arithmetic is not extended to it yet); the model stays in its previous mode. */
enum sfa_math { SFA_MATH_F32 = 0, SFA_MATH_BF16X6 = 1, SFA_MATH_FP16X3 = 2, SFA_MATH_FP16 = 3 };
int sfa_model_set_math(sfa_model* model, int math);
int sfa_model_get_math(const sfa_model* model);

/* Kernel-choice options of a model handle (no reference counterpart: the equivalence tests and
 * A/B runs of the two forms each option selects).  Every option is a field of the handle, read by
 * the forward when it enqueues its launches (a captured graph keeps the choice of its capture);
 * nothing on the launch path reads the environment.  Defaults are the production kernels; at
 * sfa_model_create the env variable named beside each key seeds it, sfa_model_set_option
 * overrides it.  Not concurrently with a forward of this model.  (Round 4: the round-2/3 tune
 * bits, stem ablations, grouped heads and second side stream — measured and not adopted — moved to
 * tools/experiments/r03 with their convbench hooks.)
 *   SFA_OPT_STEM_PATCH  (SFA_STEM_PATCH)  1 (default): the fp16x3 stem + max-pool in one kernel
 *                                         over 16 x 16 patches + a merge pass; 0: the
 *                                         implicit-GEMM stem + the max-pool kernel
 *   SFA_OPT_FPN_COMMUTE (SFA_FPN_COMMUTE) bit mask of the FPN levels run commuted (7, fp16x3)
 *   SFA_OPT_FPN_GEMM    (SFA_FPN_GEMM)    bit mask of the commuted FPN 1x1 convs on the persistent
 *                                         weight-resident kernel: bit f = level f's low-resolution
 *                                         conv, bit 3 + f = its skip conv (61: the low-res convs of
 *                                         levels 0 and 2, the level-2 skip conv on full rows, the
 *                                         level-0 / 1 skip convs on flat pixel steps); the others on
 *                                         the per-tile kernels
 *   SFA_OPT_SPLITK_TICKETS (SFA_SPLITK_TICKETS) 1 (default): the split-K layer4 strip convs combine
 *                                         their slices in the conv kernel (the last slice of a tile to
 *                                         finish, by an atomic ticket); 0: a reduce launch per conv; the
 *                                         same bits
 *   SFA_OPT_W_IMAGES    (SFA_W_IMAGES)    1 (default): the fp16x3 heads read W from the derived weight
 *                                         images (above), when the handle has them; 0: from the packed
 *                                         terms; the same bits
 *   SFA_OPT_BODY_W_IMAGES (SFA_BODY_W_IMAGES) 1 (default): the residual layers' fp16x3 strip convs read W
 *                                         from their derived weight images, when the handle has them and
 *                                         SFA_OPT_W_IMAGES is 1; 0: from the packed terms; the same bits
 */
enum sfa_model_option { SFA_OPT_STEM_PATCH = 0, SFA_OPT_FPN_COMMUTE = 1, SFA_OPT_FPN_GEMM = 2,
                        SFA_OPT_SPLITK_TICKETS = 3, SFA_OPT_W_IMAGES = 16, SFA_OPT_BODY_W_IMAGES = 17 };
int sfa_model_set_option(sfa_model* model, int key, int value);
int sfa_model_get_option(const sfa_model* model, int key, int* value);

/* Kernel probe (measurement only; no reference counterpart).  SFA_PROBE_HEADS: every
 * forward NOT being captured into a graph records a timing event before and after each
 * detection-head level's launch (the dominant kernel, 54.6 % of the FLOPs), on the stream
 * that launches it; SFA_PROBE_SERIAL: all launches stay on the caller's stream (no
 * side streams), so each head launch has the chip to itself.  sfa_model_probe_times
 * waits for the last probed forward's events and returns the launch durations of head
 * levels 0 .. n-1 in ms.  flags = 0 turns the probe off.  On a SFA_BACKBONE_DECONV model the probed
 * launches are its three transposed convolutions and its one heads launch, in that order (n <= 4). */
enum sfa_probe_flags { SFA_PROBE_HEADS = 1, SFA_PROBE_SERIAL = 2 };
int sfa_model_set_probe(sfa_model* model, int flags);
int sfa_model_probe_times(const sfa_model* model, float* ms, int n);

/* Forward.  x: device float32, layout SFA_IN_NCHW3 (B,3,H,W) as the reference
 * takes it, SFA_IN_NHWC4 (B,H,W,4) as sfa_bev_voxelize writes it, or
 * SFA_IN_NCHW3_FLIP_HW: (B,3,H,W) read as torch.flip(x, [2, 3]) — the back view of
 * utils/demo_utils.py:110-111 do_detect, fused into the layout conversion.
 * H, W multiples of 32.  head_out[i]: device float32 (B, c_i, H/4, W/4) NCHW,
 * contiguous, forward head order — raw logits like the reference (no sigmoid).
 * workspace: sfa_forward_workspace_size(B, H, W) bytes.
 * Batch limit: the conv kernels address each input map with 32-bit byte offsets, so one pass
 * holds at most sfa_forward_max_batch(H, W) frames = floor((2^31 - 1) / (32 H W)) (the widest
 * conv input, up_level3, is 32 H W bytes per frame): 181 frames at 608 x 608.  A larger batch
 * runs as consecutive passes of that many frames on the caller's stream, sharing one workspace
 * sized for a pass (bit-identical per frame: the arithmetic is batch-invariant); a single frame
 * too large for one pass (H W >= 2^26) is refused with SFA_E_UNSUPPORTED before any launch.
 * sfa_forward_max_batch is the SFA_BACKBONE_KFPN value.  sfa_model_forward_max_batch is the model's own:
 * the same for a KFPN model; for a SFA_BACKBONE_DECONV model the widest conv input is the heads'
 * 256-channel (H/4, W/4) map, 64 H W bytes per frame, so a pass holds floor((2^31 - 1) / (64 H W))
 * frames: 90 at 608 x 608 (needs a handle only, no device).  The workspace size, the pass chunking and
 * the buffer offsets of a model follow its own limit. */
enum sfa_input_layout { SFA_IN_NCHW3 = 0, SFA_IN_NHWC4 = 1, SFA_IN_NCHW3_FLIP_HW = 2 };
int sfa_forward_max_batch(int height, int width);
int sfa_model_forward_max_batch(const sfa_model* model, int height, int width);
size_t sfa_forward_workspace_size(const sfa_model* model, int batch, int height, int width);
int sfa_model_forward(const sfa_model* model, const float* x, int in_layout, int batch, int height,
                      int width, float* const* head_out, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Byte offset inside the forward workspace of an intermediate map, valid after
 * sfa_model_forward returns on the stream (for the reference's opt-in
 * visualisation capture, fpn_resnet.py:189-242).  LAYERk / UP_LEVELk are NHWC
 * float32 (B, h, w, C); HEADS_Lk are channel-planar float32
 * [sum(head_channels)][B][h][w] per KFPN level.  -1 on bad arguments.
 * Which reference tensor each buffer holds (fpn_resnet.py:184-233):
 *   LAYER1..4   out_layer1..4, (B, H/4 .. H/32, W/4 .. W/32, 64 .. 512)
 *   UP_LEVEL2   up_level2 = bilinear x2 of conv_up_level1's output, (B, H/8, W/8, 256): head level 0's input
 *   UP_LEVEL3   up_level3 = bilinear x2 of conv_up_level2's output, (B, H/4, W/4, 128): head level 1's input
 *   UP_LEVEL4   up_level4 = conv_up_level3's output itself,        (B, H/4, W/4, 64):  head level 2's input
 *   HEADS_Lk    level k's head maps BEFORE the resize and apply_kfpn, heads in forward order along the
 *               channel axis; level 0 at (H/8, W/8), levels 1, 2 at (H/4, W/4)
 * (up_level1, the concatenations and the conv_up_level1/2 outputs at their own resolution are not kept:
 * the fp16x3 forward never forms the first two.)
 * Ordering: the side stream that runs head levels 0 and 2 forks from and joins back into the caller's
 * stream inside sfa_model_forward, before the KFPN combine, on failure too; so work ordered after the
 * forward on the caller's stream (or a synchronisation of that stream alone) sees every buffer
 * complete; a device-wide synchronisation is sufficient, not required.  Another stream needs an event.
 * SFA_BACKBONE_DECONV models: LAYER1..4 as above; DECONV1..3 = the three transposed-conv stage outputs
 * after BN + ReLU (resnet.py:230 deconv_layers[2], [5], [8]), NHWC float32 (B, H/16, W/16, 256),
 * (B, H/8, W/8, 256), (B, H/4, W/4, 256) — DECONV3 is the heads' input.  UP_LEVEL* and HEADS_L* do not
 * exist there (-1), as DECONV* do not on a KFPN model (-1).
 * The offsets are those of one pass: for batch > sfa_forward_max_batch the buffers hold the last pass
 * only, at the offsets of a batch of sfa_forward_max_batch frames. */
enum sfa_buffer {
  SFA_BUF_LAYER1 = 0, SFA_BUF_LAYER2, SFA_BUF_LAYER3, SFA_BUF_LAYER4,
  SFA_BUF_UP_LEVEL2, SFA_BUF_UP_LEVEL3, SFA_BUF_UP_LEVEL4,
  SFA_BUF_HEADS_L0, SFA_BUF_HEADS_L1, SFA_BUF_HEADS_L2,
  SFA_BUF_DECONV1, SFA_BUF_DECONV2, SFA_BUF_DECONV3
};
int64_t sfa_forward_buffer_offset(const sfa_model* model, int batch, int height, int width,
                                  int which);

/* --------------------------------------------------------------- decode --
 * Replaces utils/torch_utils.py:44-45 _sigmoid (in place: sigmoid then
 * clamp(1e-4, 1-1e-4)). */
int sfa_sigmoid_clamp_inplace(float* x, int64_t n, void* stream);

/* Replaces utils/evaluation_utils.py:77-105 decode (with _nms :21-26, _topk
 * :47-62, _transpose_and_gather_feat :40-44).  All maps device float32 NCHW
 * contiguous: hm (B,C,H,W), off (B,2,H,W) or NULL, dir (B,2,H,W),
 * z (B,1,H,W), dim (B,3,H,W).  apply_sigmoid != 0 applies _sigmoid to hm and
 * off on the fly (the test.py:150,167 pair) without modifying them.
 * dets: device float32 (B, K, 10) columns
 *   [score, xs+off0, ys+off1, z, dim0, dim1, dim2, dir0, dir1, class].
 * Ties (unspecified order in torch.topk) break by lower flat index, then lower
 * class.  Constraints: K <= 256, K <= H*W, H*W <= 262144 (512 x 512, any aspect, H = 1 or W = 1
 * included), C <= 16; a larger map is SFA_E_INVALID before any launch.  dets and workspace must
 * not be hm itself (SFA_E_INVALID).
 * Maps of H*W <= 36864 run the band / whole-map kernels; larger ones (the Argoverse scripts'
 * 200 x 200 heat map of an 800 x 800 input, argoverse_test2.py:37-47) run the tiled form: a class
 * map is cut into tiles of rows and, for W > 1024, of columns, each tile's top K is selected with
 * a 1-cell halo, and the tile lists are merged per class, then per frame.  Same results, bit for bit.
 * workspace: sfa_decode_workspace_size_hw(B, C, H, W, K) bytes (0 for an unsupported shape; less
 * is SFA_E_WORKSPACE before any launch).  sfa_decode_workspace_size(B, C, K) is that value for
 * every map of H*W <= 36864 and stays sufficient for those. */
size_t sfa_decode_workspace_size(int batch, int num_classes, int K);
size_t sfa_decode_workspace_size_hw(int batch, int num_classes, int height, int width, int K);
int sfa_decode(const float* hm, const float* off, const float* dir, const float* z,
               const float* dim, int batch, int num_classes, int height, int width, int K,
               int apply_sigmoid, float* dets, void* workspace, size_t workspace_bytes,
               void* stream);

/* The reference's decode helpers, each on its own (utils/evaluation_utils.py; the drop-in
 * utils.evaluation_utils serves them from these, so no caller falls through to torch code):
 *
 * sfa_heat_nms replaces :21-26 _nms(heat, kernel=3): out = heat * (max_pool2d(heat, 3, 1, 1) ==
 * heat) over `maps` float32 maps of height x width (pool padded with -inf; non-peaks become the
 * signed zero of the multiply).  out must not alias heat.
 *
 * sfa_topk replaces :47-62 _topk(scores, K) (per_channel = 0) and :65-74 _topk_channel
 * (per_channel = 1) on float32 (B, C, H, W) scores (no peak test; decode's sfa_decode fuses it):
 *   per_channel = 0: out_scores f32 (B, K), out_inds int64 (B, K) (flat index within the class
 *     map), out_clses int32 (B, K), out_ys / out_xs f32 (B, K) = floor(ind / W), ind % W;
 *   per_channel = 1: out_scores, out_inds, out_ys, out_xs of shape (B, C, K); out_clses unused.
 * Each class's K by (value desc, index asc), then the classes' C*K by (value desc, class asc,
 * rank asc) — torch.topk's two stages, its unspecified tie order made definite.  Constraints as
 * sfa_decode (K <= 256, K <= H*W <= 262144, C <= 16; the tiled form above 36864); workspace
 * sfa_topk_workspace_size_hw(B, C, H, W, K) (= sfa_decode_workspace_size_hw;
 * sfa_topk_workspace_size(B, C, K) covers H*W <= 36864).
 *
 * sfa_gather_feat replaces :29-37 _gather_feat(feat, ind) (mask None: stride_n = dim, stride_d = 1,
 * feat (B, n, dim)) and :40-44 _transpose_and_gather_feat (feat (B, dim, H, W): n = H*W,
 * stride_n = 1, stride_d = H*W): out[b][k][d] = feat[b*n*dim + ind[b][k]*stride_n + d*stride_d],
 * elements of elem_bytes 4 (f32 / int32) or 8 (int64); ind int64 (B, K) in [0, n), checked by the
 * caller (torch.gather's contract). */
int sfa_heat_nms(const float* heat, float* out, int64_t maps, int height, int width, void* stream);
size_t sfa_topk_workspace_size(int batch, int num_classes, int K);
size_t sfa_topk_workspace_size_hw(int batch, int num_classes, int height, int width, int K);
int sfa_topk(const float* scores, int batch, int num_classes, int height, int width, int K, int per_channel,
             float* out_scores, int64_t* out_inds, int32_t* out_clses, float* out_ys, float* out_xs,
             void* workspace, size_t workspace_bytes, void* stream);
int sfa_gather_feat(const void* feat, int batch, int64_t n, int dim, int64_t stride_n, int64_t stride_d,
                    int elem_bytes, const int64_t* ind, int K, void* out, void* stream);

/* ------------------------------------------------ post-processing on device --
 * the SFA side of the fusion scripts without a host hop.
 *
 * sfa_post_process replaces utils/evaluation_utils.py:112-163 post_processing (for
 * EVERY frame; the reference returns only the last one, :158) followed by :177-193
 * convert_det_to_real_values.  dets: device f32 (B, K, 10) from sfa_decode.  Per frame
 * the rows with class == j and score > peak_thresh (f32 compare), class-major, decode
 * order within a class, are written compacted (frame b at out_offsets[b], a DEVICE
 * int32 array of batch+1 entries written by the call):
 *   out_preds f32 (n, 8) [score, x*down, y*down, z, h, w/bound_y*bev_w, l/bound_x*bev_h,
 *                         atan2(dir0, dir1)]          (the post_processing dict rows)
 *   out_real  f64 (n, 8) [class, x, y, z, h, w, l, yaw] (convert_det_to_real_values)
 * convert_det_to_real_values works on numpy scalars, so its arithmetic type follows the
 * numpy version: SFA_REAL_F32 = numpy >= 2 (f32, as the fixtures were generated),
 * SFA_REAL_F64 = numpy 1.x (f64 from the f32 inputs; requirements.txt pins 1.18.3).
 * Capacity: batch*K rows.  One workgroup (the work is a few hundred rows). */
enum sfa_real_arith { SFA_REAL_F32 = 0, SFA_REAL_F64 = 1 };
typedef struct sfa_post_params {
  int num_classes;        /* 3 */
  int down_ratio;         /* 4 */
  float peak_thresh;      /* 0.2 */
  int bev_h, bev_w;       /* 608, 608 (kitti_config.py BEV_HEIGHT / BEV_WIDTH) */
  double bound_x, bound_y;            /* 50, 50 */
  double min_x, min_y, min_z;         /* 0, -25, -2.73 */
  int arith;              /* SFA_REAL_F32 | SFA_REAL_F64 */
} sfa_post_params;
int sfa_post_process(const float* dets, int batch, int K, const sfa_post_params* params,
                     float* out_preds, double* out_real, int32_t* out_offsets, void* stream);

/* sfa_project_boxes replaces test6.py:129-187 convert_sfa3d_to_2d_boxes (with
 * data_process/transformation.py:99-107 lidar_to_camera_box): for each real row
 * (CSR by DEVICE offsets) whose confidence >= conf_min — the confidence is column 0
 * (the class id, as the reference reads it, test6.py:138) with SFA_CONF_CLASS_ID or the
 * detection score (preds column 0) with SFA_CONF_SCORE — the 8 box corners are moved
 * to the camera (V2C, R0), rotated by ry = -yaw - pi/2, projected with P2, clipped to
 * the image like Python max(0, .) / min(img, .), and kept when max > min as int32
 * [int(min_x), int(min_y), int(max_x - min_x), int(max_y - min_y)].
 * Outputs compacted per frame (out_offsets, DEVICE int32 batch+1, written by the
 * call): boxes int32 (m, 4), conf f64, out_row = the row index within the frame's
 * real rows, out_extent (optional) f64 (m, 4) = clipped [min_x, min_y, max_x, max_y].
 * calib: DEVICE array of `batch` sfa_calib (or one, when calib_per_frame = 0); the
 * matrices are the calib file's values (f32 in the reference, widened to f64).
 * f64 without contraction; numpy's BLAS and libm may differ in the last ulp. */
enum sfa_conf_source { SFA_CONF_CLASS_ID = 0, SFA_CONF_SCORE = 1 };
typedef struct sfa_calib {
  double V2C[12];  /* Tr_velo_to_cam 3x4, row-major */
  double R0[9];    /* R_rect 3x3 */
  double P2[12];   /* 3x4 */
  int32_t img_h, img_w;
} sfa_calib;
typedef struct sfa_project_params {
  double conf_min;      /* 0.3 */
  int conf_source;      /* SFA_CONF_CLASS_ID | SFA_CONF_SCORE */
  int calib_per_frame;  /* 1: calib[b] per frame; 0: calib[0] for all */
} sfa_project_params;
int sfa_project_boxes(const double* real, const float* preds, const int32_t* offsets, int batch,
                      const sfa_calib* calib, const sfa_project_params* params,
                      int32_t* out_boxes, double* out_conf, int32_t* out_row, double* out_extent,
                      int32_t* out_offsets, void* stream);

/* Argoverse: detections -> image corners (the scripts' draw_3d_bbox_on_image without the drawing).
 *
 * sfa_argo_project_boxes replaces argoverse_test2.py:432-436 (grid -> metres through the
 * boundary), :355-402 create_3d_bbox_corners and :324-353 ArgoverseCalibration.project_to_image,
 * with the draw condition of :454-458.  preds: DEVICE f32 (capacity, 8) rows
 * [score, x, y, z, h, w, l, yaw] as sfa_post_process writes them (out_preds); offsets: that call's
 * DEVICE int32 offsets (batch + 1 entries; rows [0, offsets[batch]) are processed, the rest of the
 * outputs is left untouched) or NULL (all `capacity` rows).  Per row, in float32 without
 * contraction (numpy >= 2 keeps f32 scalar arithmetic in f32):
 *   cx = maxX - x * d, cy = y * d + minY, cz = z + minZ     (boundary as sfa_argo_bev_voxelize)
 *   corner k = R_y(yaw) @ [+-l/2, 0 or -h, +-w/2] + [cx, cy, cz], k in the reference's order.
 * Each corner then goes, in float64, through T_l2c (HOST, 16 doubles, 4x4 row-major) and P2 (HOST,
 * 12 doubles, 3x4), read during the call: a corner with camera Z <= 0.1 is NaN in both
 * coordinates, the others are (P2 cam)[0:2] / (P2 cam)[2] rounded to float32.
 *   out_pixels    DEVICE f32 (capacity, 8, 2)
 *   out_all8      DEVICE int32 (capacity): 1 when all eight corners are finite (the box is drawn)
 *   out_corners3d DEVICE f32 (capacity, 8, 3) or NULL: the corners in the lidar frame
 * One thread per corner; capacity <= 2^24.
 *
 * sfa_argo_project_points is project_to_image (:324-353) on its own: points DEVICE (n, 3) float32
 * (points_f64 = 0) or float64 (1) -> out_pixels DEVICE f32 (n, 2). */
int sfa_argo_project_boxes(const float* preds, const int32_t* offsets, int batch, int capacity,
                           const double* boundary, double discretization, const double* T_l2c,
                           const double* P2, float* out_pixels, int32_t* out_all8, float* out_corners3d,
                           void* stream);
int sfa_argo_project_points(const void* points, int points_f64, int64_t n, const double* T_l2c,
                            const double* P2, float* out_pixels, void* stream);

/* ------------------------------------------------------- .bin streaming --
 * KITTI velodyne .bin files (data_process/kitti_dataset.py:119-122
 * get_lidar = np.fromfile(path, float32).reshape(-1, 4)) read in batches by a producer
 * thread with n_threads pread() workers into two host staging slots, overlapped with
 * the GPU work of the previous batch.  pinned = 1: slots are hipHostMalloc'd and
 * sfa_bin_stream_next copies a batch to DEVICE `points` with hipMemcpyAsync on
 * `stream` (the slot is reused only after that copy completed); pinned = 0: plain host
 * slots, `points` is a HOST buffer (memcpy; no device involved).  The stream allocates
 * its own host memory (2 x max_points_per_batch x 16 B), never device memory.
 * next() fills frame_offsets (HOST, batch + 1 entries, ready for sfa_bev_voxelize) and
 * *n_frames (< batch for the last partial batch, 0 at the end).  A file whose float
 * count is not a multiple of 4 fails the batch (the reference's reshape raises). */
typedef struct sfa_bin_stream sfa_bin_stream;
int sfa_bin_stream_create(const char* const* paths, int n_files, int batch,
                          int64_t max_points_per_batch, int n_threads, int pinned,
                          sfa_bin_stream** out);
int sfa_bin_stream_next(sfa_bin_stream* s, float* points, int64_t capacity_points,
                        int64_t* frame_offsets, int* n_frames, void* stream);
void sfa_bin_stream_destroy(sfa_bin_stream* s);

/* ------------------------------------------------------------ fusion --
 * Camera-LiDAR late fusion + NMS.  Replaces test6.py:310-348
 * create_fused_detections_wrapper -> :231-308 bayesian_inspired_fuse_overlapping_detections
 * (mode SFA_FUSE_BAYES) or test5.py:285-321 create_fused_detections -> :213-282
 * fuse_overlapping_detections (SFA_FUSE_WEIGHTED), then test6.py:104-126
 * apply_nms_to_fused_detections, all with test6.py:76-101 calculate_iou.
 *
 * Per frame b (CSR by DEVICE int32 offsets [batch+1]): YOLO boxes int32 [x,y,w,h],
 * f64 confidence, int32 class id; SFA 2D boxes int32 [x,y,w,h], f64 confidence.
 * At most 512 boxes per side per frame (a larger frame gets out_count = -1).
 * Output for frame b starts at element yolo_offsets[b] + sfa_offsets[b] (capacity
 * = its yolo + sfa count): the fused list in the reference's order (fused/kept YOLO
 * entries in YOLO order, then unmatched SFA), source SFA_SRC_*, class id (SFA: 0);
 * out_origin (optional) = index of the entry in its frame's INPUT list (YOLO for
 * YOLO/fused entries, SFA for SFA entries), out_match (optional) = the SFA input
 * index fused into a fused entry, else -1;
 * out_keep = indices into that list of the NMS survivors, in NMS output order.
 * All f64 arithmetic is IEEE without contraction: bit-identical to the Python. */
enum sfa_fuse_mode { SFA_FUSE_BAYES = 0, SFA_FUSE_WEIGHTED = 1 };
enum sfa_fuse_source { SFA_SRC_YOLO = 0, SFA_SRC_LIDAR = 1, SFA_FUSED = 2 };
typedef struct sfa_fusion_params {
  double conf_threshold;        /* keep detections with conf >= this (default 0.3) */
  double fusion_iou_threshold;  /* associate when IoU >= this (default 0.7) */
  double nms_threshold;         /* suppress when IoU > this (default 0.5) */
  int mode;                     /* SFA_FUSE_BAYES | SFA_FUSE_WEIGHTED */
  int apply_nms;                /* 0: fusion only */
} sfa_fusion_params;

/* IoU matrix out[i][j] = calculate_iou(a[i], b[j]) (test6.py:76-101), f64. */
int sfa_iou_matrix(const int32_t* boxes_a, int na, const int32_t* boxes_b, int nb, double* out,
                   void* stream);

/* Gaussian soft-NMS: replaces README.md:250-261 gaussian_nms(detections, sigma=0.5) (the
 * reference's only definition of it): for each frame b, the count[b] detections at
 * boxes/conf[start[b] ..] (DEVICE int32 starts/counts [batch]; boxes int32 [x,y,w,h] as
 * calculate_iou, test6.py:76-101) are visited in order and every later one decays in place,
 * conf[j] *= exp(-iou(i, j)^2 / sigma) for i < j in increasing i; order, boxes and count are
 * unchanged (no threshold).  f64; a count <= 0 leaves the frame untouched.  Chains after
 * sfa_fuse_detections with starts = yolo_offsets[b] + sfa_offsets[b], counts = out_count. */
int sfa_gaussian_nms(int batch, const int32_t* boxes, double* conf, const int32_t* starts,
                     const int32_t* counts, double sigma, void* stream);

int sfa_fuse_detections(int batch, const int32_t* yolo_boxes, const double* yolo_conf,
                        const int32_t* yolo_cls, const int32_t* yolo_offsets,
                        const int32_t* sfa_boxes, const double* sfa_conf,
                        const int32_t* sfa_offsets, const sfa_fusion_params* params,
                        int32_t* out_boxes, double* out_conf, int32_t* out_cls, int32_t* out_src,
                        int32_t* out_origin, int32_t* out_match, int32_t* out_count,
                        int32_t* out_keep, int32_t* out_keep_count, void* stream);

/* ------------------------------------------------- validation: targets + loss --
 * The reference's only quality figure is the validation loss (train.py:250-275 validate): the val
 * loader's targets, the model, losses.losses.Compute_Loss, averaged.  Evaluation only: no
 * gradient is formed anywhere.
 *
 * sfa_build_targets replaces data_process/kitti_dataset.py:157-244 KittiDataset.build_targets (with
 * kitti_data_utils.py:176-225 compute_radius, gaussian2D, gen_hm_radius) for a batch of label lists.
 *   labels         DEVICE f32 [total_rows][8] = cls, x, y, z, h, w, l, yaw, in label order
 *   frame_offsets  DEVICE int64 [batch + 1] (in rows; frame b = rows [off[b], off[b+1]), clamped to
 *                  [0, total_rows]); only the first max_objects rows of a frame are read (:165)
 *   params         boundary = minX, maxX, minY, maxY, minZ, maxZ; hm_h x hm_w the heat map
 *                  (configs.hm_size), num_classes <= 16, max_objects 1..256; bit b of the h-flip mask
 *                  (lo: frames 0..31, hi: 32..63) = frame b is flipped (:196, :225), so batch <= 64;
 *                  reserved words zero
 * Outputs, all DEVICE and all written in full by the call (nothing needs zeroing; graph-capturable):
 *   hm_cen (B, C, H, W) f32, cen_offset (B, M, 2) f32, direction (B, M, 2) f32, z_coor (B, M, 1) f32,
 *   dim (B, M, 3) f32, indices_center (B, M) int64, obj_mask (B, M) uint8, status uint32 [B].
 * Semantics are the reference's loop, label by label: yaw = -yaw; the boundary test and the
 * h, w, l <= 0 test leave the slot zero; radius = max(0, int(compute_radius(ceil(l'), ceil(w'))));
 * centre, its h-flip, center_int = trunc; the gaussian of diameter 2r + 1 and sigma = diameter / 6 in
 * float64, clipped at the map edges, combined with max; a label with cls < 0 (-1: every class,
 * otherwise class -cls - 2) draws its gaussian at center_int, then ASSIGNS 0.9999 at the centre cell
 * and fills no slot.  The assignment makes the map depend on the label order; each cell is computed
 * by walking the labels in that order, so any order is exact.  Float dtypes follow numpy >= 2 (a
 * float32 scalar combined with a Python number stays float32; tests/loss_restatement.py states every
 * step); the float64 exp / sin / cos may differ from libm's by an ulp, i.e. in the float32 result
 * only at a rounding midpoint.
 * status bit 0: a centre fell outside the map (x == maxX gives center_int[1] == hm_h; a flipped
 * y == maxY gives center_int[0] == -1): the gaussian is clipped like the reference's slices, the index
 * the reference computes is stored, the 0.9999 of an ignore label (where the reference raises or
 * wraps) is not written, nothing is written out of bounds.  bit 1: a class id >= num_classes or
 * < -num_classes - 1 (the reference raises IndexError); the row is skipped.
 * SFA_E_INVALID before any launch: batch, classes, H or W <= 0, classes > 16, max_objects outside
 * 1..256, batch > 64, H*W > 2^24, nonzero reserved words, a NULL pointer. */
typedef struct sfa_target_params {
  double boundary[6];
  int hm_h, hm_w, num_classes, max_objects;
  uint32_t hflip_mask_lo, hflip_mask_hi;
  int reserved[6];
} sfa_target_params;
int sfa_build_targets(const float* labels, const int64_t* frame_offsets, int64_t total_rows, int batch,
                      const sfa_target_params* params, float* hm_cen, float* cen_offset,
                      float* direction, float* z_coor, float* dim, int64_t* indices_center,
                      uint8_t* obj_mask, uint32_t* status, void* stream);

/* sfa_compute_loss replaces losses/losses.py:128-163 Compute_Loss.forward (FocalLoss / _neg_loss
 * :44-69, L1Loss :83-92, L1Loss_Balanced :95-125 with alpha 0.5, gamma 1.5, beta 1; unit weights).
 * The five head maps are DEVICE f32 NCHW as sfa_model_forward writes them ((B, C | 2 | 2 | 1 | 3, H, W));
 * the targets are sfa_build_targets' tensors.  apply_sigmoid as in sfa_decode: 1 applies _sigmoid
 * (sigmoid, clamp to [1e-4, 1 - 1e-4], sfa_sigmoid_clamp_inplace's arithmetic) to hm_cen and
 * cen_offset on the fly without writing them back, 0 takes them as clamped probabilities.
 *   loss    DEVICE f32 [6] = total, hm_cen, cen_offset, dim, direction, z_coor (the loss_stats order)
 *   sums    DEVICE f64 [8] = focal positive sum, negative sum, num_pos, the masked sums of
 *           cen_offset, dim, direction, z_coor, and the mask sum (objects)
 *   status  DEVICE uint32 [1]: bit 0 = a slot with a set mask has an index outside [0, H*W) (the
 *           reference's gather raises); the slot contributes nothing
 * Every term is evaluated in float64 from the float32 operands and summed in float64 in an order
 * fixed by the shape (per-block partials in the workspace, one folding launch; no floating-point
 * atomics): runs are bit-identical.  hm_cen = -neg when num_pos == 0, else -(pos + neg) / num_pos;
 * an L1 term = sum / (mask sum * channels + 1e-4); the six values are rounded to float32 once.
 * workspace: DEVICE, 8-byte aligned, sfa_compute_loss_workspace_size(B, C, H, W, M) bytes (0 for a
 * shape out of range: B 1..64, C 1..16, M 1..256, H*W <= 2^24), SFA_E_WORKSPACE when smaller. */
size_t sfa_compute_loss_workspace_size(int batch, int num_classes, int height, int width, int max_objects);
int sfa_compute_loss(const float* hm_cen, const float* cen_offset, const float* direction,
                     const float* z_coor, const float* dim, const float* t_hm_cen,
                     const float* t_cen_offset, const float* t_direction, const float* t_z_coor,
                     const float* t_dim, const int64_t* indices_center, const uint8_t* obj_mask, int batch,
                     int num_classes, int height, int width, int max_objects, int apply_sigmoid,
                     float* loss, double* sums, uint32_t* status, void* workspace, size_t workspace_bytes,
                     void* stream);

/* sfa_compute_loss_grad: the gradient of sfa_compute_loss's total (unit weights) with respect to the
 * five head maps; what total_loss.backward() leaves at the heads (train.py:190-247).  Inputs and
 * shape limits are sfa_compute_loss's.  Outputs: five DEVICE f32 NCHW maps of the inputs' shapes,
 * every byte written by the call (a cell no slot points at gets 0.0; nothing needs zeroing).
 * apply_sigmoid 1: g_hm_cen and g_cen_offset are taken with respect to the logits (the focal / L1
 * derivative times s (1 - s) where 1e-4 <= s <= 1 - 1e-4, both ends included, 0 elsewhere, s being
 * sfa_sigmoid_clamp_inplace's float32 sigmoid); 0: with respect to the clamped probabilities.
 * With p the probability, k = -1 / num_pos (-1 when num_pos == 0), m the slot's mask, d = pred m - t m
 * and S the mask sum (slots with an index inside the map):
 *   hm_cen      gt == 1: k [(1-p)^2 / p - 2 (1-p) log p];  gt < 1: k (1-gt)^4 [2 p log(1-p) - p^2 / (1-p)]
 *   cen_offset, direction   sign(d) m / (2 S + 1e-4) at the slot's cell, sign(0) = 0
 *   z_coor, dim             sign(d) m (0.5 log((e^3 - 1) |d| + 1) if |d| < 1 else 1.5) / (c S + 1e-4), c = 1, 3
 * Slots of one frame that share a cell add up, in slot order.  Evaluated in float64 from the float32
 * operands, rounded to float32 once per element; no floating-point atomics: runs are bit-identical.
 *   status  DEVICE uint32 [1], bit 0 as in sfa_compute_loss (the slot contributes nothing)
 * workspace: DEVICE, 8-byte aligned, sfa_compute_loss_grad_workspace_size(B, C, H, W, M) bytes (0 for
 * a shape out of range), SFA_E_WORKSPACE when smaller.  Three launches on the caller's stream, no
 * allocation, no synchronisation: graph-capturable. */
size_t sfa_compute_loss_grad_workspace_size(int batch, int num_classes, int height, int width,
                                            int max_objects);
int sfa_compute_loss_grad(const float* hm_cen, const float* cen_offset, const float* direction,
                          const float* z_coor, const float* dim, const float* t_hm_cen,
                          const float* t_cen_offset, const float* t_direction, const float* t_z_coor,
                          const float* t_dim, const int64_t* indices_center, const uint8_t* obj_mask,
                          int batch, int num_classes, int height, int width, int max_objects,
                          int apply_sigmoid, float* g_hm_cen, float* g_cen_offset, float* g_direction,
                          float* g_z_coor, float* g_dim, uint32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---------------------------------------- apply_kfpn as an operator: forward + gradient --
 * For a detector built in torch that trains against sfa_compute_loss_grad: the last operator between
 * the 15 per-level head outputs and the five head maps.  sfa_model_forward keeps its own fused
 * combine; these two entries take the user-facing layouts and cover every head in one launch each.
 *
 * sfa_kfpn_combine replaces models/fpn_resnet.py:248-254 apply_kfpn for all heads, with the nearest
 * resize of level 0 (:229-230) read in place.
 *   levels       HOST array [3 * num_heads] of DEVICE f32 pointers, head-major: head j's levels 0, 1, 2 at
 *                3 j, 3 j + 1, 3 j + 2.  Levels 1 and 2 are NCHW (B, channels[j], h, w), contiguous;
 *                level 0 too when level0_half == 0, and (B, channels[j], h / 2, w / 2) when
 *                level0_half == 1, read by nearest resize (src = dst / 2: F.interpolate(size=(h, w)) at an
 *                exact 0.5 scale; h and w even)
 *   channels     HOST int [num_heads], each > 0; num_heads 1 .. SFA_MAX_HEADS
 *   out          HOST array [num_heads] of DEVICE f32 (B, channels[j], h, w)
 *   weights      NULL, or HOST array [num_heads] of DEVICE f32 (B, channels[j], h, w, 3): the softmax
 *                over the three levels, apply_kfpn's second return value
 * Per element, in float32 without contraction and in sfa_model_forward's order: mx = max(v0, v1, v2),
 * e_i = expf(v_i - mx), s = e0 + e1 + e2, w_i = e_i / s, out = v0 w0 + v1 w1 + v2 w2: given the same level
 * values the result is bit-identical to sfa_model_forward's head maps.
 *
 * sfa_kfpn_combine_grad: the gradient of a scalar `total` at the 3 * num_heads level maps given
 * grad_out[j] = d total / d out[j] (DEVICE f32, out's shape):
 *   d total / d v_j = g w_j (1 + v_j - out),  w = softmax(v), out = sum_i v_i w_i
 * evaluated in float64 from the float32 operands and rounded to float32 once.  grad_levels: HOST array
 * [3 * num_heads] of DEVICE f32 maps of the levels' shapes.  Under level0_half a level-0 cell receives
 * the sum of its four children's terms, added in float64 in the order (0,0), (0,1), (1,0), (1,1) (row,
 * column) by the thread that owns the cell: no atomics, nothing needs zeroing, every byte of every
 * gradient map is written, runs are bit-identical.
 *
 * Both: one launch on the caller's stream, no workspace, no allocation, no synchronisation
 * (graph-capturable).  128-bit loads and stores when w % 4 == 0 and every DEVICE pointer is 16-byte
 * aligned, scalar ones otherwise, with the same bits.  SFA_E_INVALID before any launch: a NULL array or
 * entry, num_heads outside 1 .. SFA_MAX_HEADS, B, h, w or a channel count <= 0, level0_half not 0 / 1, odd
 * h or w under level0_half, B or the channel sum above 65535, h w above 2^30. */
int sfa_kfpn_combine(const float* const* levels, const int* channels, int num_heads, int B, int h, int w,
                     int level0_half, float* const* out, float* const* weights, void* stream);
int sfa_kfpn_combine_grad(const float* const* levels, const int* channels, int num_heads, int B, int h,
                          int w, int level0_half, const float* const* grad_out,
                          float* const* grad_levels, void* stream);

/* ------------------------------------------- head parameter gradients (one KFPN level) --
 * What total_loss.backward() leaves at the parameters of the level's heads, fpn{level}_{head}.0.weight,
 * .0.bias, .2.weight, .2.bias (models/fpn_resnet.py:135-143 conv3x3 -> ReLU -> conv1x1; train.py:190-247),
 * given g = d total / d y, the level's head outputs, as sfa_kfpn_combine_grad writes them.  With x the
 * heads' input, A = conv3x3(x; W1) + b1, Hd = max(A, 0), y = W2 Hd + b2:
 *   db2[c] = sum_{b,p} g[b,c,p]                    dW2[c,o] = sum_{b,p} g[b,c,p] Hd[b,p,o]
 *   dA[b,p,o] = Hd[b,p,o] > 0 ? sum_c W2[c,o] g[b,c,p] : 0   (strict, torch's ReLU backward)
 *   db1[o] = sum_{b,p} dA[b,p,o]
 *   dW1[o,i,ky,kx] = sum_{b,y,x} dA[b,y,x,o] x[b,y+ky-1,x+kx-1,i], zero outside the map
 * The gradient with respect to x is a separate entry, sfa_model_heads_input_grad below, on the dA this one writes to
 * dhidden_out (fine-tuning the heads on a frozen backbone needs none).
 *   model, level   a SFA_BACKBONE_KFPN handle and its level 0, 1, 2: Cin = 256, 128, 64 and the level's head
 *                  weights inside the handle (SFA_BACKBONE_DECONV: SFA_E_UNSUPPORTED)
 *   x              DEVICE f32 (B, h, w, Cin) NHWC, 16-byte aligned: SFA_BUF_UP_LEVEL2 / 3 / 4 after a forward,
 *                  or any caller buffer; h, w any positive sizes
 *   grad_levels    HOST array [num_heads] of DEVICE f32 (B, c_j, h, w) NCHW, forward head order
 *   grad_w1/b1/w2/b2  HOST arrays [num_heads] of DEVICE f32 (64, Cin, 3, 3), (64), (c_j, 64, 1, 1), (c_j):
 *                  torch's own layouts, every byte written by the call
 *   hidden_out, dhidden_out   NULL, or DEVICE f32 (B, h, w, 64 num_heads), 16-byte aligned: Hd and dA as the
 *                  kernels used them (head j's channels at 64 j ..); NULL keeps them in the workspace
 *   max_chunk_pixels  0: the plan's choice (4096); > 0 caps the pixels of one split-K chunk of dW1.  A chunk
 *                  is a run of whole rows of one frame, at least one row
 *   workspace      DEVICE, 16-byte aligned, sfa_model_heads_grad_workspace_size(...) bytes (0 for arguments
 *                  the entry refuses); smaller: SFA_E_WORKSPACE
 * Arithmetic.  Hd is recomputed by the fp16x3 convolution (SFA_MATH_FP16X3, the forward's default arithmetic)
 * whatever sfa_model_set_math says, with every frame of x scaled by its own max |x|, which the call measures: it
 * may differ from the forward's own hidden activation in the last bits (another kernel, another summation order),
 * and in the sign of a pre-activation that close to zero.  dA, dW2, db1, db2: float64 from the float32
 * operands, rounded once (per-block partials added in block order).  dW1: v_mfma_f32_32x32x2_f32 with
 * float32 accumulation inside one chunk, the chunks added in chunk order in float64, rounded once;
 * sfa_model_heads_grad_chunk_pixels returns K_c, the largest chunk's pixel count, which is the K of the
 * float32 part (0 for arguments the entry refuses).
 * Eight launches (seven for an even head count) on the caller's stream; no allocation, no synchronisation, no memset, no floating-point
 * atomics; two runs are bit-identical; graph-capturable.  Before any launch: SFA_E_INVALID for a NULL
 * pointer, a level outside 0..2, non-positive B, h or w, negative max_chunk_pixels, a misaligned buffer, or
 * B h w max(Cin, 64 num_heads) 4 >= 2^31 (32-bit byte offsets); SFA_E_WORKSPACE for a short workspace. */
size_t sfa_model_heads_grad_workspace_size(const sfa_model* model, int level, int B, int h, int w,
                                           int max_chunk_pixels);
int sfa_model_heads_grad_chunk_pixels(const sfa_model* model, int level, int B, int h, int w,
                                      int max_chunk_pixels);
int sfa_model_heads_grad(const sfa_model* model, int level, const float* x, int B, int h, int w,
                         const float* const* grad_levels, float* const* grad_w1, float* const* grad_b1,
                         float* const* grad_w2, float* const* grad_b2, float* hidden_out, float* dhidden_out,
                         int max_chunk_pixels, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------- the heads as an operator (one KFPN level) --
 * sfa_model_heads_input_grad: the gradient at the heads' input x, summed over the level's heads (every head
 * reads the same x), from dA (B, h, w, 64 num_heads) as sfa_model_heads_grad writes it to dhidden_out:
 *   dX[b,y,x,i] = sum_o sum_{ky,kx} dA[b, y+1-ky, x+1-kx, o] W1[o,i,ky,kx]     (dA zero outside the map)
 *   dhidden, grad_x   DEVICE f32 (B, h, w, 64 num_heads) and (B, h, w, Cin) NHWC, 16-byte aligned
 * One launch on the caller's stream: an implicit GEMM on v_mfma_f32_32x32x2_f32 whose whole K = 9 * 64 num_heads
 * is walked inside one workgroup per tile of sfa_heads_dgrad_pixel_tile() pixels of one image row x 64 input
 * channels, accumulated in float32 in a fixed order.  No workspace, no partial tiles, no atomics, no memset;
 * every byte of grad_x is written; two runs are bit-identical; graph-capturable.
 *
 * sfa_model_heads_forward: the level's heads on a caller's x: Hd = ReLU(conv3x3(x; W1) + b1) by the very launches
 * sfa_model_heads_grad recomputes it with (fp16x3, the frames' own max |x|), so for the same x the two Hd are
 * bit-equal and a ReLU edge falls the same way in the forward and in the gradient; then y = W2 Hd + b2 per pixel
 * and channel in float64 from the float32 operands (b2 first, the 64 products in hidden-channel order), rounded
 * once.  y is NOT promised bit-equal to sfa_model_forward's level maps: those come from another kernel (the
 * fused head epilogue) with another summation order.
 *   y_levels     HOST array [num_heads] of DEVICE f32 (B, c_j, h, w) NCHW, forward head order, every byte written
 *   hidden_out   NULL, or DEVICE f32 (B, h, w, 64 num_heads), 16-byte aligned: Hd
 *   workspace    DEVICE, 16-byte aligned, sfa_model_heads_forward_workspace_size(...) bytes (0 for arguments the
 *                entry refuses); smaller: SFA_E_WORKSPACE
 * Five launches (four for an even head count) on the caller's stream; graph-capturable.
 *
 * Both, before any launch: SFA_E_INVALID for a NULL pointer, a level outside 0..2, non-positive B, h or w, a
 * misaligned buffer, or B h w max(Cin, 64 num_heads) 4 >= 2^31; SFA_E_UNSUPPORTED for a SFA_BACKBONE_DECONV model. */
int sfa_heads_dgrad_pixel_tile(void);
int sfa_model_heads_input_grad(const sfa_model* model, int level, const float* dhidden, int B, int h, int w,
                               float* grad_x, void* stream);
size_t sfa_model_heads_forward_workspace_size(const sfa_model* model, int level, int B, int h, int w);
int sfa_model_heads_forward(const sfa_model* model, int level, const float* x, int B, int h, int w,
                            float* const* y_levels, float* hidden_out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ------------------------------------------- the FPN neck as an operator (fpn_resnet_18) --
 * models/fpn_resnet.py:197-210: three 1x1 convolutions with bias over cat(up(x), skip) and three bilinear x2
 * (align_corners=True) resizes, no BatchNorm, no non-linearity.  All maps are DEVICE float32 NHWC, 16-byte
 * aligned: l4 (B, h4, w4, 512), l3 (B, 2 h4, 2 w4, 256), l2 (B, 4 h4, 4 w4, 128), l1 (B, 8 h4, 8 w4, 64) in;
 * u2 (B, 4 h4, 4 w4, 256), u3 (B, 8 h4, 8 w4, 128), u4 (B, 8 h4, 8 w4, 64) = up_level2 / 3 / 4.  W_f, b_f are
 * conv_up_level{f}.weight / .bias as float32 inside the handle; U is the resize as the model's own forward
 * evaluates it (float32 source index scale * o, scale 0 for a one-row or one-column source):
 *   z1 = W1 cat(U l4, l3) + b1,  u2 = U z1;   z2 = W2 cat(u2, l2) + b2,  u3 = U z2;   u4 = W3 cat(u3, l1) + b3
 *
 * sfa_model_neck_forward: U l4 is written to the workspace, each convolution is one pointwise GEMM on
 * v_mfma_f32_32x32x2_f32 (rows = sfa_neck_pixel_tile() flat pixels, K = the input channels read as two segments,
 * no concat buffer, bias in the epilogue), each resize one launch of the forward's kernel: six launches.  The
 * arithmetic is float32 MFMA; u2 / u3 / u4 are NOT promised bit-equal to sfa_model_forward's maps, which come
 * from the fused fp16x3 FPN stage.
 *
 * sfa_model_neck_grad: from g2, g3, g4 = d total / d u2, u3, u4 (g2 and g3 may be NULL: zero; g4 is required)
 *   dZ3 = g4            dW3 = dZ3^T cat(u3, l1)   db3 = sum dZ3   d_l1 = dZ3 W3b   d_u3 = g3 + dZ3 W3a
 *   dZ2 = U^T d_u3      dW2 = dZ2^T cat(u2, l2)   db2 = sum dZ2   d_l2 = dZ2 W2b   d_u2 = g2 + dZ2 W2a
 *   dZ1 = U^T d_u2      dW1b = dZ1^T l3           db1 = sum dZ1   d_l3 = dZ1 W1b
 *   dL  = U^T dZ1       dW1a = dL^T l4                            d_l4 = dL W1a
 * (Wfa: the first, "up", input columns of W_f; Wfb the rest; U and a 1x1 convolution commute, so stage 1's up
 * half runs at l4's resolution.)  U^T is a gather: every low-resolution element adds, in float64 in (row, column)
 * order, the high-resolution elements whose footprint reaches it, times the float32 coefficients the forward's
 * kernel computes for that pixel, rounded once.  The data gradients walk their whole K (<= 256) inside one
 * workgroup; the weight gradients are split-K over chunks of flat pixels (max_chunk_pixels caps a chunk, 0: the
 * plan's own size) whose float32 partial tiles a fold adds in chunk order in float64, rounded once; the bias
 * gradients are float64 sums in pixel order, rounded once.
 *   d_l1 .. d_l4   each NULL (not wanted) or the shape of l1 .. l4; every byte written
 *   dparams        NULL, or a HOST array of 6 DEVICE pointers dW1 (256, 768), db1 (256), dW2 (128, 384), db2 (128),
 *                  dW3 (64, 192), db3 (64) in torch's layouts, each may be NULL; every byte written
 *   l1 .. l4, u2, u3   read only by the weight gradients: NULL is allowed for the maps no wanted output reads
 *                  (all of them when dparams is NULL)
 *   workspace      DEVICE, 16-byte aligned, sfa_model_neck_grad_workspace_size(...) bytes (0 for refused arguments)
 * sfa_model_neck_grad_chunk_pixels(f = 1, 2, 3) is K_c of dW_f, the pixels of its largest chunk: the K of the
 * longest float32 accumulation, which the error bound of dW_f uses.  No atomics, no memset, nothing allocates or
 * synchronises; two runs are bit-identical; graph-capturable.
 *
 * Both entries, before any launch: SFA_E_INVALID for a NULL required pointer, a NULL g4, no output wanted,
 * non-positive B, h4 or w4, a negative max_chunk_pixels, a misaligned buffer, a workspace that is too small, or a
 * shape whose largest map passes 2^31 bytes; SFA_E_UNSUPPORTED for a SFA_BACKBONE_DECONV model (it has no neck). */
int sfa_neck_pixel_tile(void);
size_t sfa_model_neck_forward_workspace_size(const sfa_model* model, int B, int h4, int w4);
int sfa_model_neck_forward(const sfa_model* model, const float* l1, const float* l2, const float* l3, const float* l4,
                           int B, int h4, int w4, float* u2, float* u3, float* u4, void* workspace,
                           size_t workspace_bytes, void* stream);
size_t sfa_model_neck_grad_workspace_size(const sfa_model* model, int B, int h4, int w4, int max_chunk_pixels);
int sfa_model_neck_grad_chunk_pixels(const sfa_model* model, int f, int B, int h4, int w4, int max_chunk_pixels);
int sfa_model_neck_grad(const sfa_model* model, const float* l1, const float* l2, const float* l3, const float* l4,
                        const float* u2, const float* u3, const float* g2, const float* g3, const float* g4, int B,
                        int h4, int w4, float* d_l1, float* d_l2, float* d_l3, float* d_l4, float* const* dparams,
                        int max_chunk_pixels, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------- one BasicBlock as an operator (fpn_resnet_18, layer1..4) --
 * models/fpn_resnet.py:42-71 with every BatchNorm as the handle holds it: running statistics, folded into the
 * convolution before it (W' = s W, b' = beta - mean s, s = gamma / sqrt(var + 1e-5)).  Block layer{layer}.{block},
 * layer = 1..4, block = 0, 1: Cout = 64 2^(layer-1); for block == 0 && layer > 1 the stride s is 2, Cin = Cout / 2
 * and the skip is the 1x1 stride-2 downsample, else s = 1, Cin = Cout and the skip is x itself.  All maps are DEVICE
 * float32 NHWC, 16-byte aligned: x (B, h, w, Cin); mid, y, gy (B, oh, ow, Cout), oh = ceil(h / s), ow = ceil(w / s).
 *   mid = ReLU(conv3x3_s(x; W1') + b1')
 *   y   = ReLU(conv3x3_1(mid; W2') + b2' + skip),   skip = x  or  conv1x1_s(x; Wd')   (b2' holds both BN shifts)
 *
 * sfa_model_block_forward: the model's own convolution launches in fp16x3 whatever the handle's math mode is, each
 * frame scaled by its own max |x| (and max |mid|), which the call measures; mid_out and y_out are both written.
 * Any positive h and w, odd ones at stride 2 included (the launches read the input's and the output's sizes
 * separately).  workspace: sfa_model_block_forward_workspace_size(...) bytes.
 *
 * sfa_model_block_grad: from gy = d total / d y and the maps the caller passes (the ReLU masks are read from them)
 *   dZ  = y > 0 ? gy : 0       db2' = sum dZ     dW2' = wgrad_1(dZ, mid)     dApost = dgrad_1(dZ; W2')
 *   dA  = mid > 0 ? dApost : 0 db1' = sum dA     dW1' = wgrad_s(dA, x)       dWd' = wgrad1x1_s(dZ, x)
 *   dx  = dgrad_s(dA; W1') + (dZ  or  dgrad1x1_s(dZ; Wd'))
 * on v_mfma_f32_32x32x2_f32.  dZ is never stored: the mask is applied where gy is loaded; dA's mask and the + dZ
 * term sit in the data gradients' epilogues; the 1x1 downsample is the centre tap of the 3x3 window, a second K
 * segment of the same kernels.  The data gradients walk their whole K (9 Cout, + Cout with a downsample) inside
 * one workgroup in (tap, channel) order; the weight gradients are split-K over chunks of output pixels
 * (max_chunk_pixels caps a chunk, 0: the plan's own size) whose float32 partial tiles a fold adds in chunk order in
 * float64, rounded once; the bias gradients are float64 sums in pixel order, rounded once.
 *   grad_x       NULL (not wanted) or (B, h, w, Cin); every byte written
 *   dparams      NULL, or a HOST array of 5 DEVICE pointers dW1' (Cout, Cin, 3, 3), db1' (Cout), dW2' (Cout, Cout, 3, 3),
 *                db2' (Cout), dWd' (Cout, Cin, 1, 1) in torch's layouts, each may be NULL; dWd' must be NULL on a
 *                block without a downsample; every byte of a wanted output is written
 *   x            may be NULL when neither dW1' nor dWd' is wanted; mid, y, gy are required
 *   h, w         any positive sizes, odd ones included
 *   workspace    DEVICE, 16-byte aligned, sfa_model_block_grad_workspace_size(...) bytes (0 for refused arguments)
 * sfa_model_block_grad_chunk_pixels(which = 0: dW1', 1: dW2', 2: dWd') is K_c, the pixels of that gradient's largest
 * chunk: the K of its longest float32 accumulation (0 when refused, or which = 2 without a downsample).
 * No atomics, no memset, nothing allocates or synchronises; two runs are bit-identical; graph-capturable.
 *
 * All of these, before any launch: SFA_E_INVALID for a NULL required pointer, no output wanted, layer outside 1..4,
 * block outside 0..1, non-positive B, h or w, a negative max_chunk_pixels, a misaligned buffer, a workspace that is
 * too small, a dWd' pointer on a block without a downsample, or a map of 2^31 bytes or more; SFA_E_UNSUPPORTED for a
 * SFA_BACKBONE_DECONV model.
 *
 * sfa_bn_unfold_grad: the gradients of a convolution weight W (Cout, K) and of the BatchNorm after it from the
 * gradients dWf (Cout, K), dbf (Cout) of their folded form, in float64 from the float32 operands, rounded once:
 *   s = gamma / sqrt(var + eps)    dW[o][k] = s[o] dWf[o][k]    dbeta = dbf
 *   dgamma[o] = (sum_k W[o][k] dWf[o][k] - mean[o] dbf[o]) / sqrt(var[o] + eps)
 * dW, dgamma, dbeta: each NULL or a DEVICE buffer, every element written; an operand no wanted output reads may be
 * NULL.  One launch, fixed summation order.  SFA_E_INVALID: Cout or K <= 0, Cout K >= 2^29, a negative eps, no
 * output wanted, or a NULL operand that a wanted output reads. */
size_t sfa_model_block_forward_workspace_size(const sfa_model* model, int layer, int block, int B, int h, int w);
int sfa_model_block_forward(const sfa_model* model, int layer, int block, const float* x, int B, int h, int w,
                            float* mid_out, float* y_out, void* workspace, size_t workspace_bytes, void* stream);
size_t sfa_model_block_grad_workspace_size(const sfa_model* model, int layer, int block, int B, int h, int w,
                                           int max_chunk_pixels);
int sfa_model_block_grad_chunk_pixels(const sfa_model* model, int layer, int block, int which, int B, int h, int w,
                                      int max_chunk_pixels);
int sfa_model_block_grad(const sfa_model* model, int layer, int block, const float* x, const float* mid, const float* y,
                         const float* gy, int B, int h, int w, float* grad_x, float* const* dparams,
                         int max_chunk_pixels, void* workspace, size_t workspace_bytes, void* stream);
int sfa_bn_unfold_grad(const float* W, const float* gamma, const float* mean, const float* var, double eps,
                       const float* dWf, const float* dbf, int Cout, int K, float* dW, float* dgamma, float* dbeta,
                       void* stream);

/* ------------------------- one BasicBlock in training mode: BatchNorm with batch statistics (layer1..4) --
 * models/fpn_resnet.py:42-71 under model.train(): every BatchNorm normalises with the mean and the biased variance
 * of the batch and is differentiated through them.  The entries take NO model handle (a handle holds folded fp16
 * terms packed on the host, and training changes the weights every step): the caller passes the raw float32
 * parameters in torch's layouts.  Geometry comes from (layer, block) as in sfa_model_block_*; all maps are DEVICE
 * float32 NHWC, 16-byte aligned: x (B, h, w, Cin); z1, mid, z2, zd, y, gy (B, oh, ow, Cout).  n = B oh ow is what one
 * channel of a BatchNorm sees.
 *   z1 = conv3x3_s(x; W1)            mean1, var1 = the batch mean and biased variance of z1 per channel
 *   mid = ReLU(s1 z1 + t1)           s = gamma / sqrt(var + eps),  t = beta - mean s
 *   z2 = conv3x3_1(mid; W2)          mean2, var2
 *   zd = conv1x1_s(x; Wd)            meand, vard        (block 0 of layer2..4 only)
 *   y  = ReLU(s2 z2 + t2 + (x  or  sd zd + td))
 *   params   HOST array of 9 DEVICE pointers W1 (Cout, Cin, 3, 3), gamma1, beta1, W2 (Cout, Cout, 3, 3), gamma2,
 *            beta2, Wd (Cout, Cin, 1, 1), gammad, betad; the last three NULL on a block without a downsample
 *   stats    DEVICE float32 [nbn][2][Cout], nbn = 2 (3 with a downsample): mean then biased variance of BatchNorm
 *            1, 2 and the downsample's; the forward writes it, the gradient reads it
 *
 * sfa_block_train_forward writes z1, mid, z2, zd (NULL exactly on a block without a downsample), y and stats, every
 * byte.  The convolutions are float32 on v_mfma_f32_32x32x2_f32, K in (tap, channel) order inside one workgroup, from
 * k-major copies of the weights rebuilt in the workspace every call.  The statistics are float64 sums of z and z^2
 * over blocks of pixels in pixel order, then over the blocks in block order (at most 256; max_chunk_pixels > 0 also
 * caps a block): mean = S1 / n, var = max(S2 / n - mean^2, 0), each rounded once to float32.  s and t are computed
 * once per channel in float64 FROM THE ROUNDED mean and var and rounded once; each BatchNorm is then one float32 FMA
 * per element, the skip one float32 addition, then the ReLU.
 *
 * sfa_block_train_grad: from gy = d total / d y, the maps and the statistics the forward wrote, with
 * dY = y > 0 ? gy : 0 and invstd = 1 / sqrt(var + eps), per BatchNorm
 *   dbeta = sum dY     dgamma = invstd sum dY (z - mean)
 *   dZ = gamma invstd (dY - sum dY / n - (z - mean) invstd^2 sum dY (z - mean) / n)
 * (the two sums in float64 in the statistics' block order; dZ in float64 per element, rounded once, stored in the
 * workspace), then
 *   dW2 = wgrad_1(dZ2, mid)          dA  = mid > 0 ? dgrad_1(dZ2; W2) : 0       dZ1 = BatchNorm 1's backward of dA
 *   dW1 = wgrad_s(dZ1, x)            dWd = wgrad1x1_s(dZd, x)
 *   dx  = dgrad_s(dZ1; W1) + (dY  or  dgrad1x1_s(dZd; Wd))
 * through sfa_model_block_grad's data- and weight-gradient kernels (split-K chunks of at most max_chunk_pixels
 * output pixels, 0: the plan's own size).
 *   grad_x       NULL (not wanted) or (B, h, w, Cin); every byte written
 *   dparams      NULL, or a HOST array of 9 DEVICE pointers dW1, dgamma1, dbeta1, dW2, dgamma2, dbeta2, dWd,
 *                dgammad, dbetad in torch's shapes, each may be NULL; the last three must be NULL on a block without
 *                a downsample; every byte of a wanted output is written
 *   params       as in the forward; the betas are not read and may be NULL
 * sfa_block_train_chunk_pixels(which = 0: dW1, 1: dW2, 2: dWd) is K_c, the pixels of that gradient's largest chunk;
 * which = 3 is the pixels of one statistics block (0 when refused, or which = 2 without a downsample).
 * No atomics, no memset, nothing allocates or synchronises; two runs are bit-identical; graph-capturable.
 *
 * All of these, before any launch: SFA_E_INVALID for a NULL required pointer, no output wanted, layer outside 1..4,
 * block outside 0..1, non-positive B, h or w, a negative max_chunk_pixels, a negative eps, a misaligned buffer, a
 * workspace that is too small, a downsample pointer on a block without one (zd, dWd, dgammad, dbetad; the forward
 * also refuses its parameters Wd, gammad, betad there, the gradient never reads them), a map of 2^31 bytes or more, or n < 2
 * (torch: "Expected more than 1 value per channel when training"; the size functions return 0). */
size_t sfa_block_train_forward_workspace_size(int layer, int block, int B, int h, int w, int max_chunk_pixels);
size_t sfa_block_train_grad_workspace_size(int layer, int block, int B, int h, int w, int max_chunk_pixels);
int sfa_block_train_chunk_pixels(int layer, int block, int which, int B, int h, int w, int max_chunk_pixels);
int sfa_block_train_forward(int layer, int block, const float* x, const float* const* params, double eps, int B, int h,
                            int w, float* z1, float* mid, float* z2, float* zd, float* y, float* stats,
                            int max_chunk_pixels, void* workspace, size_t workspace_bytes, void* stream);
int sfa_block_train_grad(int layer, int block, const float* x, const float* z1, const float* mid, const float* z2,
                         const float* zd, const float* y, const float* gy, const float* stats,
                         const float* const* params, double eps, int B, int h, int w, float* grad_x,
                         float* const* dparams, int max_chunk_pixels, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ------------------------- the stem in training mode: bn1 with batch statistics, float32 conv1 --
 * models/fpn_resnet.py:179-182 under model.train(): bn1 normalises with the mean and the biased variance of the batch
 * and is differentiated through them.  As sfa_block_train_*, the entries take NO model handle and read the raw float32
 * parameters in torch's layouts.  x is DEVICE float32 (B, 3, H, W) NCHW; the maps are DEVICE float32 NHWC; all 16-byte
 * aligned.  oh = ceil(H / 2), ow = ceil(W / 2), ph = ceil(oh / 2), pw = ceil(ow / 2); n = B oh ow is what one channel
 * of bn1 sees.
 *   z = conv7x7_2(x; W)                 (B, oh, ow, 64), raw: no bias, no ReLU
 *   mean, var = the batch mean and biased variance of z per channel
 *   a = ReLU(s z + t)                   s = gamma / sqrt(var + eps),  t = beta - mean s
 *   p = maxpool3x3_2(a)                 (B, ph, pw, 64)
 *   params   HOST array of 3 DEVICE pointers W (64, 3, 7, 7), gamma (64), beta (64)
 *   stats    DEVICE float32 [2][64]: mean then biased variance; the forward writes it, the gradient reads it
 *
 * sfa_stem_train_forward writes z, a, pooled and stats, every byte.  The convolution is float32 on
 * v_mfma_f32_32x32x2_f32, 64 conv pixels x 64 channels per workgroup, K = the 147 (c, ky, kx) entries in torch's
 * order (padded with zero rows to 160) inside one workgroup, the image gathered with every row and column tested,
 * from a k-major copy of W rebuilt in the workspace every call.  Statistics, (s, t) and the apply are
 * sfa_block_train_forward's, word for word: float64 sums of z and z^2 over blocks of pixels in pixel order, then over
 * the blocks in block order (at most 256; max_chunk_pixels > 0 also caps a block), mean and var each rounded once to
 * float32, s and t in float64 FROM THE ROUNDED mean and var, rounded once, one float32 FMA per element, the ReLU.
 * The max-pool is the model's own launch.
 *
 * sfa_stem_train_grad: from gp = d total / d p and the maps and statistics the forward wrote
 *   dY = a > 0 ? (pool adjoint of gp by first maximum) : 0          (sfa_model_stem_grad's adjoint)
 *   dbeta = sum dY     dgamma = invstd sum dY (z - mean)             invstd = 1 / sqrt(var + eps)
 *   dZ = gamma invstd (dY - sum dY / n - (z - mean) invstd^2 sum dY (z - mean) / n)
 *   dW = wgrad_2(dZ, x) (64, 3, 7, 7)   dx = dgrad_2(dZ; W) (B, 3, H, W)     (W is the raw weight: nothing to unfold)
 * with the two sums in float64 in the statistics' block order, dZ in float64 per element, rounded once, stored in the
 * workspace, and dW / dx through sfa_model_stem_grad's kernels (split-K chunks of at most max_chunk_pixels conv
 * pixels, 0: the plan's own size; dx from a [o][tap][4] copy of W rebuilt in the workspace).
 *   grad_x       NULL (not wanted) or (B, 3, H, W); every byte written
 *   dparams      NULL, or a HOST array of 3 DEVICE pointers dW, dgamma, dbeta in torch's shapes, each may be NULL;
 *                every byte of a wanted output is written
 *   params       as in the forward; beta is not read and may be NULL
 *   x            may be NULL when dW is not wanted; z, a, gp and stats are required
 * sfa_stem_train_chunk_pixels(which = 0) is K_c, the pixels of dW's largest chunk; which = 1 is the pixels of one
 * statistics block (0 when refused).  No atomics, no memset, nothing allocates or synchronises; two runs are
 * bit-identical; graph-capturable.
 *
 * All of these, before any launch: SFA_E_INVALID for a NULL required pointer, no output wanted, non-positive B, H or
 * W, a negative max_chunk_pixels, a negative eps, a misaligned buffer, a workspace that is too small, a map of 2^31
 * bytes or more (x counted at 16 bytes per pixel, and a), or n < 2 (the size functions return 0);
 * SFA_E_UNSUPPORTED for B above 65535 or H above 262140 (the max-pool launch puts the frame and the pooled row on
 * grid axes).  W has no limit of its own, and the 32760 of sfa_model_stem_forward's fp16x3 launch does not apply. */
size_t sfa_stem_train_forward_workspace_size(int B, int H, int W, int max_chunk_pixels);
size_t sfa_stem_train_grad_workspace_size(int B, int H, int W, int max_chunk_pixels);
int sfa_stem_train_chunk_pixels(int which, int B, int H, int W, int max_chunk_pixels);
int sfa_stem_train_forward(const float* x, const float* const* params, double eps, int B, int H, int W, float* z,
                           float* a, float* pooled, float* stats, int max_chunk_pixels, void* workspace,
                           size_t workspace_bytes, void* stream);
int sfa_stem_train_grad(const float* x, const float* z, const float* a, const float* gp, const float* stats,
                        const float* const* params, double eps, int B, int H, int W, float* grad_x,
                        float* const* dparams, int max_chunk_pixels, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------- the stem as an operator (both backbone families) --
 * models/fpn_resnet.py:179-182 on a caller's image, bn1 as the handle holds it: running statistics, folded into conv1
 * (W' = s W, b' = beta - mean s, s = gamma / sqrt(var + 1e-5)).  x is DEVICE float32 (B, 3, H, W) NCHW (SFA_IN_NCHW3;
 * the other two input layouts are not part of this operator); the maps are DEVICE float32 NHWC; all 16-byte aligned.
 *   a = ReLU(conv7x7_2(x; W') + b')   (B, oh, ow, 64), oh = ceil(H / 2), ow = ceil(W / 2)
 *   p = maxpool3x3_2(a)               (B, ph, pw, 64), ph = ceil(oh / 2), pw = ceil(ow / 2)
 *
 * sfa_model_stem_forward: the model's own unfused launches (the layout pass with its per-frame max |x|, the fp16x3
 * convolution whatever the handle's math mode is, the max-pool); a_out and pooled_out are both written.  Accepted
 * sizes: 1 <= H, W <= 32760 (the convolution launch packs input rows and columns in 16 bits), 1 <= B <= 65535 (the
 * frame is a grid axis of the layout and max-pool launches), odd sizes included, and every map below 2^31 bytes
 * (x as (B, H, W, 4) and a).  workspace: sfa_model_stem_forward_workspace_size(...) bytes.
 *
 * sfa_model_stem_grad: from gp = d total / d p (B, ph, pw, 64) and the map a the forward wrote
 *   dAp = pool adjoint of gp: a pixel of a receives a window's gp exactly when it is that window's first maximum in
 *         row-major scan order (torch's rule: strict >, padding is -inf and never wins); window maxima are recomputed
 *         from a, the pooled map is not an input
 *   dA  = a > 0 ? dAp : 0     db' = sum dA     dW' = wgrad_2(dA, x) (64, 3, 7, 7)     dx = dgrad_2(dA; W') (B, 3, H, W)
 * dA is a gather over the pixels of a (at most 4 windows per pixel), written once to the workspace; dW' runs on
 * v_mfma_f32_32x32x2_f32, split-K over chunks of conv output pixels (max_chunk_pixels caps a chunk, 0: the plan's own
 * size) whose float32 partial tiles a fold adds in chunk order in float64, rounded once; db' is a float64 sum in pixel
 * order, rounded once; dx is a vector gather over the taps of matching parity in (ky, kx, channel) order, float64
 * accumulation of exact products, rounded once, and runs only when grad_x is wanted.
 *   grad_x       NULL (not wanted) or (B, 3, H, W); every byte written
 *   dparams      NULL, or a HOST array of 2 DEVICE pointers dW' (64, 3, 7, 7) in torch's layout and db' (64), each may
 *                be NULL; every byte of a wanted output is written
 *   x            may be NULL when dW' is not wanted; a and gp are required
 *   workspace    DEVICE, 16-byte aligned, sfa_model_stem_grad_workspace_size(...) bytes (0 for refused arguments)
 * sfa_model_stem_grad_chunk_pixels is K_c, the pixels of dW's largest chunk: the K of its longest float32
 * accumulation (0 when refused).  No atomics, no memset, nothing allocates or synchronises; two runs are
 * bit-identical; graph-capturable.  NaN in a or gp is outside the contract (a NaN never counts as a maximum here).
 *
 * All of these, before any launch: SFA_E_INVALID for a NULL required pointer, no output wanted, non-positive B, H or
 * W, a negative max_chunk_pixels, a misaligned buffer, a workspace that is too small, or a map of 2^31 bytes or more;
 * SFA_E_UNSUPPORTED for H or W above 32760 or B above 65535.  A SFA_BACKBONE_DECONV handle is accepted: the stem is
 * shared code and shared packing. */
size_t sfa_model_stem_forward_workspace_size(const sfa_model* model, int B, int H, int W);
int sfa_model_stem_forward(const sfa_model* model, const float* x, int B, int H, int W, float* a_out, float* pooled_out,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t sfa_model_stem_grad_workspace_size(const sfa_model* model, int B, int H, int W, int max_chunk_pixels);
int sfa_model_stem_grad_chunk_pixels(const sfa_model* model, int B, int H, int W, int max_chunk_pixels);
int sfa_model_stem_grad(const sfa_model* model, const float* x, const float* a, const float* gp, int B, int H, int W,
                        float* grad_x, float* const* dparams, int max_chunk_pixels, void* workspace,
                        size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SFA_HIP_H_ */
