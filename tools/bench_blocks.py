#!/usr/bin/env python3
"""Per-block time of sfa_model_block_forward and sfa_model_block_grad (all outputs) at 16 frames with a 152 x 152
pooled map: the median of 50 graph replays each, beside the time of the plan's own byte traffic at the measured
device copy rate and of its arithmetic at the f32 MFMA rate.  Prints one JSON line.

Traffic model (bytes, every map counted once per kernel that reads or writes it, weights once per launch):
  forward   x + mid written + mid read + x (the skip) + y
  gradient  db2' (gy, y), dW2' (gy, y, mid + partials written and read), dWd' (gy, y, x), dA (gy, y, mid, dA),
            db1' (dA), dW1' (dA, x + partials), dx (dA, + gy, y for the skip, dx)
Arithmetic: 2 flops per multiply-add the kernels issue, the stride-2 data gradient's zero rows included."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"))
from sfa_hip import _lib, runtime, synthetic  # noqa: E402

MFMA_F32_FLOPS = 157.3e12  # MI355X peak FP32 matrix rate (public specification)
B, H0, REPLAYS = 16, 152, 50


def replay_us(fn, gpu):
    fn()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPLAYS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    gpu = torch.device("cuda", 0)
    arch = _lib.make_arch(dict(runtime.DEFAULT_HEADS))
    eng = runtime.KfpnEngine(arch, runtime.pack_state_dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), 2), arch), gpu)
    src, dst = torch.empty(1 << 28, dtype=torch.uint8, device=gpu), torch.empty(1 << 28, dtype=torch.uint8, device=gpu)
    copy_rate = 2 * src.numel() / (replay_us(lambda: dst.copy_(src), gpu) * 1e-6)  # read + write bytes per second
    del src, dst
    out = {"frames": B, "pooled": [H0, H0], "replays": REPLAYS, "copy_GBps": round(copy_rate / 1e9, 1),
           "mfma_f32_TFLOPs": MFMA_F32_FLOPS / 1e12, "blocks": {}}
    h = H0
    gen = torch.Generator().manual_seed(1)
    for layer in (1, 2, 3, 4):
        for block in (0, 1):
            cin, cout, s, ds = eng.block_shape(layer, block)
            oh = -(-h // s)
            x = torch.randn((B, h, h, cin), generator=gen).to(gpu)
            fws = torch.empty(eng.block_forward_workspace_bytes(layer, block, B, h, h), dtype=torch.uint8, device=gpu)
            mid, y = eng.block_forward(layer, block, x)
            gy = torch.randn(y.shape, generator=gen).to(gpu)
            fwd = replay_us(lambda: eng.block_forward(layer, block, x, out=(mid, y), workspace=fws), gpu)
            gws = torch.empty(eng.block_grad_workspace_bytes(layer, block, B, h, h), dtype=torch.uint8, device=gpu)
            dx, dp = eng.block_grad(layer, block, x, mid, y, gy)
            grad = replay_us(lambda: eng.block_grad(layer, block, x, mid, y, gy, out=(dx, dp), workspace=gws), gpu)
            nin, nout = B * h * h, B * oh * oh
            X, M = 4 * nin * cin, 4 * nout * cout  # bytes of x and of one output-sized map
            kc = eng.block_grad_chunk_pixels(layer, block, 0, B, h, h)
            chunks = -(-nout // kc)
            w1, w2, wd = 4 * cout * 9 * cin, 4 * cout * 9 * cout, (4 * cout * cin if ds else 0)
            fbytes = X + M + M + X + M + w1 + w2 + wd
            gbytes = (2 * M) + (3 * M + 2 * chunks * w2) + ((2 * M + X + 2 * chunks * wd) if ds else 0) + (4 * M + w2) \
                + M + (M + X + 2 * chunks * w1) + (M + 2 * M + X + w1 + wd)
            fflops = 2 * nout * cout * (9 * cin + 9 * cout + (cin if ds else 0))
            gflops = 2 * nout * cout * 9 * cout + 2 * nin * cin * (9 + (1 if ds else 0)) * cout \
                + 2 * nout * cout * (9 * cin + 9 * cout + (cin if ds else 0))
            out["blocks"][f"layer{layer}.{block}"] = {
                "in": [h, h, cin], "out": [oh, oh, cout], "forward_us": round(fwd, 1), "grad_us": round(grad, 1),
                "forward_traffic_us": round(fbytes / copy_rate * 1e6, 1), "forward_mfma_f32_us": round(fflops / MFMA_F32_FLOPS * 1e6, 1),
                "grad_traffic_us": round(gbytes / copy_rate * 1e6, 1), "grad_mfma_f32_us": round(gflops / MFMA_F32_FLOPS * 1e6, 1)}
            h = oh
    print(json.dumps(out))


if __name__ == "__main__":
    main()
