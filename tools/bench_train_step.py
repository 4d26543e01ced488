#!/usr/bin/env python3
"""Times of the differentiable stem and of one whole training step.  Prints one JSON line.

  stem_forward, stem_grad (all outputs, and without dx): the median of 50 graph replays at 16 frames of 608 x 608,
  beside the time of the plan's own byte traffic at the measured device copy rate and of the issued arithmetic at the
  f32 MFMA rate (tools/bench_blocks.py's two yardsticks).
  train step: detect_from_image -> Compute_Loss -> backward(), eager, the median of 5 after one warm-up, at the largest
  power-of-two batch of 608 x 608 frames (16 at most) that fits next to the saved activations; the JSON says which.

Traffic model (bytes, every map counted once per kernel that reads or writes it):
  forward   x read, x as NHWC4 written and read, a written, a read, pooled written
  gradient  dA (a, gp read, dA written), db' (dA), dW' (dA, x + partials written and read), dx (dA read, dx written)
Arithmetic: 2 flops per multiply-add issued: forward 64 x 196 per conv pixel (the packed K with its zero fourth
channel), dW' 64 x 192 per conv pixel (147 columns padded to three tiles), dx 3 x 64 x the live taps per image pixel
(12.25 on average) in float64 on the vector unit, shown against the same f32 MFMA yardstick.

  block rows (--blocks adds them, --blocks-only prints them alone): layer1.1 at 16 frames of 152 x 152 and layer2.0
  at 152 x 152 -> 76 x 76, training-mode forward + gradient (sfa_block_train_forward / sfa_block_train_grad, batch
  statistics) beside the running-statistics operator's (sfa_model_block_forward / sfa_model_block_grad) from the same
  job, each the median of 50 graph replays.  Training-mode traffic, M = one (npix_out, Cout) map, X = x:
    forward   per convolution: its input read, z written, z read by the statistics; the two applies: z read, the skip
              (X or zd) read, mid / y written
    gradient  per BatchNorm: the reduce reads g, the mask and z, the apply reads them again and writes dZ; dW2 (dZ2,
              mid), dA (dZ2, mid, dA written), dW1 (dZ1, X), dx (dZ1, [dZd | gy, y], dx written), dWd (dZd, X)
  Arithmetic: 2 Cout 9 Cin (+ Cout Cin) flops per output pixel forward, twice that for the gradient (dW and the data
  gradient of each convolution), against the f32 MFMA rate.

  weight update (--weight-update-only prints these alone): weight_update_us = KfpnEngine.repack (sfa_pack_weights_device
  + sfa_model_refresh_weight_images), the median of 50 graph replays, beside the time of its byte traffic at the copy
  rate: the state read once, the packed buffer and both image buffers written, the fp16 terms the image build reads
  (the size of the images again).  weight_update_host_us = the host route, eager: pack_state_dict(model.state_dict())
  + KfpnEngine(...) + one synchronise, the median of 5.  weight_update_eager_us = the device route eager, as a step
  loop pays it: _engine() after an in-place change plus one synchronise, weight_update_eager_host_us its part until the
  call returns (the pointer table, the argument checks, the launches), the median of 5.  The train step is followed by torch.optim.Adam's step (lr 1e-3,
  no weight decay) and the next forward's _engine(), wall-clock with a synchronise each, as fields of their own.

  --stem-train adds the training-mode stem (sfa_stem_train_forward / sfa_stem_train_grad, bn1 on batch statistics,
  conv1 in float32) from the same job, each the median of 50 graph replays, and ``train_step_batch_stats_us``: the
  train step once more with backbone_trainable(batch_stats=True).  Traffic, X = x as NCHW3, A = one (npix_a, 64) map,
  P = the pooled map:
    forward   conv (X read, z written), statistics (z), apply (z read, a written), pool (a read, P written)
    gradient  dY (a, gp read, dY written), the reduce (dY, z), the apply (dY, z read, dZ written), dW (dZ, X + partials
              written and read), dx (dZ read, dx written)
  Arithmetic: forward 64 x 160 per conv pixel (the 147 entries padded to ten steps), dW and dx as above."""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"))
sys.path.insert(0, HERE)
from bench_blocks import MFMA_F32_FLOPS, REPLAYS, replay_us  # noqa: E402
from sfa_hip import _lib, runtime, synthetic  # noqa: E402

B, H = 16, 608


def train_step_us(gpu, sd, batch, batch_stats=False):
    from losses.losses import Compute_Loss
    from models.fpn_resnet import get_pose_net
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, False)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(gpu).eval().backbone_trainable(batch_stats=batch_stats)
    x = torch.from_numpy(synthetic.synthetic_bev(batch, H, H, seed=3)).to(gpu)
    labels, offsets = synthetic.synthetic_labels(batch, seed=2)
    tg = runtime.TargetBuilder(gpu, hm_size=(H // 4, H // 4))(labels, offsets)
    crit = Compute_Loss(gpu, differentiable=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=0)
    ts, ts_opt, ts_eng = [], [], []
    for it in range(6):
        for p in m.parameters():
            p.grad = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        total, _ = crit(dict(m(x)), tg)
        total.backward()
        b.record()
        b.synchronize()
        t0 = time.perf_counter()
        opt.step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        m._engine(gpu)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if it:
            ts.append(a.elapsed_time(b) * 1e3)
            ts_opt.append((t1 - t0) * 1e6)
            ts_eng.append((t2 - t1) * 1e6)
    return float(np.median(ts)), float(np.median(ts_opt)), float(np.median(ts_eng))


def weight_update_rows(gpu, sd, arch, copy_rate):
    from models.fpn_resnet import get_pose_net
    layout = _lib.state_layout(arch)
    tensors = [torch.zeros((), dtype=torch.int64, device=gpu) if n.endswith("num_batches_tracked")
               else torch.from_numpy(np.asarray(sd[n], np.float32)).to(gpu) for n, _ in layout]
    eng = runtime.KfpnEngine.from_state(arch, tensors, gpu)
    dev = replay_us(lambda: eng.repack(tensors), gpu)
    pack_only = replay_us(lambda: runtime._pack_on_device(arch, tensors, eng.weights, _lib.stream_ptr(gpu)), gpu)
    state_bytes = 4 * sum(t.numel() for t in tensors if t.is_floating_point())
    images = eng.weight_image_bytes() + eng.body_weight_image_bytes()
    traffic = state_bytes + 4 * eng.weights.numel() + 2 * images
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, False)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(gpu).eval()
    host = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e = runtime.KfpnEngine(arch, runtime.pack_state_dict(m.state_dict(), arch), gpu)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
        del e
    # the same update eager, as a step loop pays it: _engine() after an in-place change, the host's share (the pointer
    # table, the argument checks, the launches) until the call returns and the whole until the device is done
    kept = m._engine(gpu)
    eager_host, eager = [], []
    for _ in range(6):
        with torch.no_grad():
            m.conv1.weight.add_(0.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert m._engine(gpu) is kept
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        eager_host.append((t1 - t0) * 1e6)
        eager.append((time.perf_counter() - t0) * 1e6)
    return {"weight_update_eager_us": round(float(np.median(eager[1:])), 1),
            "weight_update_eager_host_us": round(float(np.median(eager_host[1:])), 1),
            "weight_update_us": round(dev, 1), "weight_pack_only_us": round(pack_only, 1),
            "weight_update_traffic_us": round(traffic / copy_rate * 1e6, 1), "weight_update_bytes": traffic,
            "weight_update_host_us": round(float(np.median(host)), 1)}


def block_rows(gpu, eng, copy_rate):
    rows = {}
    us = lambda v, rate: round(v / rate * 1e6, 1)  # noqa: E731
    for layer, block in ((1, 1), (2, 0)):
        cin, cout, s, ds = eng.block_shape(layer, block)
        h = 152
        gen = torch.Generator().manual_seed(layer)
        x = torch.randn((B, h, h, cin), generator=gen).to(gpu)
        mods = [(cout, cin, 3), (cout, cout, 3)] + ([(cout, cin, 1)] if ds else [])
        ps = []
        for co, ci, k in mods:
            ps += [(torch.randn((co, ci, k, k), generator=gen) / (k * k * ci) ** 0.5).to(gpu),
                   torch.rand(co, generator=gen).add(0.5).to(gpu), torch.randn(co, generator=gen).mul(0.3).to(gpu)]
        m = runtime.block_train_forward(layer, block, x, ps)
        gy = torch.randn(m["y"].shape, generator=gen).to(gpu)
        fws = torch.empty(runtime.block_train_forward_workspace_bytes(layer, block, B, h, h), dtype=torch.uint8, device=gpu)
        gws = torch.empty(runtime.block_train_grad_workspace_bytes(layer, block, B, h, h), dtype=torch.uint8, device=gpu)
        dx, dp = runtime.block_train_grad(layer, block, x, m, gy, ps)
        tf = replay_us(lambda: runtime.block_train_forward(layer, block, x, ps, out={k: v for k, v in m.items() if v is not None},
                                                           workspace=fws), gpu)
        tg = replay_us(lambda: runtime.block_train_grad(layer, block, x, m, gy, ps, out=(dx, dp), workspace=gws), gpu)
        mid, y = eng.block_forward(layer, block, x)
        ews = torch.empty(eng.block_forward_workspace_bytes(layer, block, B, h, h), dtype=torch.uint8, device=gpu)
        egws = torch.empty(eng.block_grad_workspace_bytes(layer, block, B, h, h), dtype=torch.uint8, device=gpu)
        edx, edp = eng.block_grad(layer, block, x, mid, y, gy)
        ef = replay_us(lambda: eng.block_forward(layer, block, x, out=(mid, y), workspace=ews), gpu)
        eg = replay_us(lambda: eng.block_grad(layer, block, x, mid, y, gy, out=(edx, edp), workspace=egws), gpu)
        npo = m["y"].numel() // cout
        M, X = 4 * npo * cout, 4 * x.numel()
        fbytes = (X + 2 * M) + (3 * M) + (2 * M) + (2 * M + (M if ds else X)) + ((X + 2 * M) if ds else 0)
        nbn = 3 if ds else 2
        gbytes = nbn * (3 * M + 4 * M) + 2 * M + 3 * M + (M + X) + (M + (M if ds else 2 * M) + X) + ((M + X) if ds else 0)
        flops = 2 * npo * cout * (9 * cin + 9 * cout + (cin if ds else 0))
        name = f"layer{layer}.{block}"
        rows[name] = {"in": [B, h, h, cin], "train_forward_us": round(tf, 1), "train_grad_us": round(tg, 1),
                      "train_forward_traffic_us": us(fbytes, copy_rate), "train_grad_traffic_us": us(gbytes, copy_rate),
                      "train_forward_mfma_f32_us": us(flops, MFMA_F32_FLOPS), "train_grad_mfma_f32_us": us(2 * flops, MFMA_F32_FLOPS),
                      "running_stats_forward_us": round(ef, 1), "running_stats_grad_us": round(eg, 1)}
    return rows


def main():
    gpu = torch.device("cuda", 0)
    arch = _lib.make_arch(dict(runtime.DEFAULT_HEADS))
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 2)
    eng = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    src, dst = torch.empty(1 << 28, dtype=torch.uint8, device=gpu), torch.empty(1 << 28, dtype=torch.uint8, device=gpu)
    copy_rate = 2 * src.numel() / (replay_us(lambda: dst.copy_(src), gpu) * 1e-6)  # read + write bytes per second
    del src, dst
    if "--weight-update-only" in sys.argv:
        print(json.dumps({"replays": REPLAYS, "copy_GBps": round(copy_rate / 1e9, 1),
                          **weight_update_rows(gpu, sd, arch, copy_rate)}))
        return
    if "--blocks-only" in sys.argv:
        print(json.dumps({"frames": B, "replays": REPLAYS, "copy_GBps": round(copy_rate / 1e9, 1),
                          "mfma_f32_TFLOPs": MFMA_F32_FLOPS / 1e12, "blocks": block_rows(gpu, eng, copy_rate)}))
        return
    x = torch.from_numpy(synthetic.synthetic_bev(B, H, H, seed=3)).to(gpu)
    fws = torch.empty(eng.stem_forward_workspace_bytes(B, H, H), dtype=torch.uint8, device=gpu)
    a, pooled = eng.stem_forward(x)
    gp = torch.randn(pooled.shape, generator=torch.Generator().manual_seed(1)).to(gpu)
    fwd = replay_us(lambda: eng.stem_forward(x, out=(a, pooled), workspace=fws), gpu)
    gws = torch.empty(eng.stem_grad_workspace_bytes(B, H, H), dtype=torch.uint8, device=gpu)
    dx, dp = eng.stem_grad(x, a, gp)
    grad = replay_us(lambda: eng.stem_grad(x, a, gp, out=(dx, dp), workspace=gws), gpu)
    grad_nodx = replay_us(lambda: eng.stem_grad(x, a, gp, want_x=False, out=(None, dp), workspace=gws), gpu)
    nx, na = B * H * H, B * (H // 2) ** 2
    X3, X4, A, P = 12 * nx, 16 * nx, 256 * na, 64 * na
    chunks = -(-na // eng.stem_grad_chunk_pixels(B, H, H))
    part = 2 * chunks * 64 * 147 * 4
    fbytes = X3 + 2 * X4 + 2 * A + P
    g_nodx = (A + P + A) + A + (A + X3 + part)
    gbytes = g_nodx + A + X3
    fflops = 2 * na * 64 * 196
    wflops = 2 * na * 64 * 192
    xflops = 2 * nx * 3 * 64 * 12.25
    us = lambda v, rate: round(v / rate * 1e6, 1)  # noqa: E731
    out = {"frames": B, "image": [H, H], "replays": REPLAYS, "copy_GBps": round(copy_rate / 1e9, 1),
           "mfma_f32_TFLOPs": MFMA_F32_FLOPS / 1e12,
           "stem_forward_us": round(fwd, 1), "stem_forward_traffic_us": us(fbytes, copy_rate),
           "stem_forward_mfma_f32_us": us(fflops, MFMA_F32_FLOPS),
           "stem_grad_us": round(grad, 1), "stem_grad_traffic_us": us(gbytes, copy_rate),
           "stem_grad_flops_us": us(wflops + xflops, MFMA_F32_FLOPS),
           "stem_grad_without_dx_us": round(grad_nodx, 1), "stem_grad_without_dx_traffic_us": us(g_nodx, copy_rate),
           "stem_grad_without_dx_mfma_f32_us": us(wflops, MFMA_F32_FLOPS), "dx_us": round(grad - grad_nodx, 1)}
    if "--stem-train" in sys.argv:
        ps = [torch.from_numpy(np.asarray(sd[k])).to(gpu) for k in ("conv1.weight", "bn1.weight", "bn1.bias")]
        tf = torch.empty(runtime.stem_train_forward_workspace_bytes(B, H, H), dtype=torch.uint8, device=gpu)
        tg = torch.empty(runtime.stem_train_grad_workspace_bytes(B, H, H), dtype=torch.uint8, device=gpu)
        tm = runtime.stem_train_forward(x, ps)
        tdx, tdp = runtime.stem_train_grad(x, tm, gp, ps)
        t_fwd = replay_us(lambda: runtime.stem_train_forward(x, ps, out=tm, workspace=tf), gpu)
        t_grad = replay_us(lambda: runtime.stem_train_grad(x, tm, gp, ps, out=(tdx, tdp), workspace=tg), gpu)
        t_nodx = replay_us(lambda: runtime.stem_train_grad(x, tm, gp, ps, want_x=False, out=(None, tdp), workspace=tg), gpu)
        tchunks = -(-na // runtime.stem_train_chunk_pixels(0, B, H, H))
        tfb = (X3 + A) + A + 2 * A + (A + P)
        tg_nodx = (A + P + A) + 2 * A + 3 * A + (A + X3 + 2 * tchunks * 64 * 147 * 4)
        out.update({"stem_train_forward_us": round(t_fwd, 1), "stem_train_forward_traffic_us": us(tfb, copy_rate),
                    "stem_train_forward_mfma_f32_us": us(2 * na * 64 * 160, MFMA_F32_FLOPS),
                    "stem_train_grad_us": round(t_grad, 1), "stem_train_grad_traffic_us": us(tg_nodx + A + X3, copy_rate),
                    "stem_train_grad_flops_us": us(wflops + xflops, MFMA_F32_FLOPS),
                    "stem_train_grad_without_dx_us": round(t_nodx, 1),
                    "stem_train_grad_without_dx_traffic_us": us(tg_nodx, copy_rate)})
        del ps, tf, tg, tm, tdx, tdp
    del x, a, pooled, gp, dx, dp, fws, gws
    if "--blocks" in sys.argv:
        out["blocks"] = block_rows(gpu, eng, copy_rate)
    batch = B
    while batch >= 1:
        torch.cuda.empty_cache()
        try:
            step, opt_us, eng_us = train_step_us(gpu, sd, batch)
            out["train_step_us"], out["optimizer_step_us"], out["engine_update_us"] = round(step, 1), round(opt_us, 1), round(eng_us, 1)
            if "--stem-train" in sys.argv:
                torch.cuda.empty_cache()
                out["train_step_batch_stats_us"] = round(train_step_us(gpu, sd, batch, batch_stats=True)[0], 1)
            break
        except torch.cuda.OutOfMemoryError:
            batch //= 2
    out["train_step_frames"] = batch
    torch.cuda.empty_cache()
    out.update(weight_update_rows(gpu, sd, arch, copy_rate))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
