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
(12.25 on average) in float64 on the vector unit, shown against the same f32 MFMA yardstick."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"))
sys.path.insert(0, HERE)
from bench_blocks import MFMA_F32_FLOPS, REPLAYS, replay_us  # noqa: E402
from sfa_hip import _lib, runtime, synthetic  # noqa: E402

B, H = 16, 608


def train_step_us(gpu, sd, batch):
    from losses.losses import Compute_Loss
    from models.fpn_resnet import get_pose_net
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, False)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(gpu).eval().backbone_trainable()
    x = torch.from_numpy(synthetic.synthetic_bev(batch, H, H, seed=3)).to(gpu)
    labels, offsets = synthetic.synthetic_labels(batch, seed=2)
    tg = runtime.TargetBuilder(gpu, hm_size=(H // 4, H // 4))(labels, offsets)
    crit = Compute_Loss(gpu, differentiable=True)
    ts = []
    for it in range(6):
        for p in m.parameters():
            p.grad = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        total, _ = crit(dict(m(x)), tg)
        total.backward()
        b.record()
        b.synchronize()
        if it:
            ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    gpu = torch.device("cuda", 0)
    arch = _lib.make_arch(dict(runtime.DEFAULT_HEADS))
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 2)
    eng = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    src, dst = torch.empty(1 << 28, dtype=torch.uint8, device=gpu), torch.empty(1 << 28, dtype=torch.uint8, device=gpu)
    copy_rate = 2 * src.numel() / (replay_us(lambda: dst.copy_(src), gpu) * 1e-6)  # read + write bytes per second
    del src, dst
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
    del x, a, pooled, gp, dx, dp, fws, gws
    batch = B
    while batch >= 1:
        torch.cuda.empty_cache()
        try:
            out["train_step_us"] = round(train_step_us(gpu, sd, batch), 1)
            break
        except torch.cuda.OutOfMemoryError:
            batch //= 2
    out["train_step_frames"] = batch
    print(json.dumps(out))


if __name__ == "__main__":
    main()
