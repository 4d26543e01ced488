"""Timing of the plain resnet_18 detector (models/resnet.py; SFA_BACKBONE_DECONV), which bench.py (fixed
on the KFPN model) does not cover.

    python tools/bench_arch.py [--batch 16] [--steps 50] [--warmup 10]

Forward + _sigmoid + decode(K=50) of `batch` 608 x 608 synthetic frames, captured in one HIP graph and
replayed: `warmup` untimed replays (clocks, caches), then `steps` timed ones between two events -> frames/s.
Then one eager serial pass with the library's kernel probe (sfa_model_set_probe: events around the three
transposed-conv launches and the fused-heads launch, each with the chip to itself), repeated `steps` times,
median per launch in us, and each launch's fraction of the fp16x3 matrix ceiling (MACs x 2 x 3 products
over the dense fp16 MFMA peak).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"))

PEAK_FP16_MFMA_TFLOPS = 2500.0  # dense fp16 MFMA, MI355X
H = W = 608


def launch_macs(batch, num_heads=5):
    """MACs per launch: deconv i reads (H/32 2^i)^2 pixels x 4 phases x (4 Cin) x 256; the heads' 3 x 3 conv."""
    out = []
    for i, cin in enumerate((512, 256, 256)):
        px = (H // 32 << i) * (W // 32 << i)
        out.append(batch * px * 4 * 4 * cin * 256)
    out.append(batch * (H // 4) * (W // 4) * 9 * 256 * 64 * num_heads)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--weight-seed", type=int, default=2)
    a = ap.parse_args()
    import torch
    from sfa_hip import _lib, runtime, synthetic
    dev = torch.device("cuda", 0)
    heads = runtime.DEFAULT_HEADS
    arch = _lib.make_arch(heads, backbone=_lib.BACKBONE_DECONV)
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), a.weight_seed)
    eng = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), dev)
    B = a.batch
    x = torch.from_numpy(synthetic.synthetic_bev(B, H, W, seed=1)).to(dev)
    outs = eng.alloc_outputs(B, H, W)
    ws = torch.empty(eng.workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    dec = runtime.Decoder()
    dets = torch.empty((B, 50, 10), dtype=torch.float32, device=dev)
    dws = torch.empty(dec.workspace_bytes(B, heads["hm_cen"], 50), dtype=torch.uint8, device=dev)

    def step():
        eng.forward_into(x, outs, workspace=ws)
        return dec(outs["hm_cen"], outs["cen_offset"], outs["direction"], outs["z_coor"], outs["dim"], K=50,
                   apply_sigmoid=True, out=dets, workspace=dws)

    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for _ in range(a.warmup):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    # serial pass: per-launch events (eager; the probe never records while a stream is being captured)
    eng.set_probe(_lib.PROBE_HEADS | _lib.PROBE_SERIAL)
    per = [[] for _ in range(4)]
    for i in range(a.warmup + a.steps):
        eng.forward_into(x, outs, workspace=ws)
        t = eng.probe_times(4)
        if i >= a.warmup:
            for k in range(4):
                per[k].append(t[k] * 1e3)
    eng.set_probe(0)
    macs = launch_macs(B, len(heads))
    names = ["deconv1", "deconv2", "deconv3", "heads"]
    launches = {}
    for k, n in enumerate(names):
        us = statistics.median(per[k])
        tf = macs[k] * 2 * 3 / (us * 1e-6) / 1e12
        launches[n] = {"us": round(us, 1), "min_us": round(min(per[k]), 1), "gmac": round(macs[k] / 1e9, 2),
                       "fp16x3_tflops": round(tf, 1), "fraction_of_ceiling": round(tf / PEAK_FP16_MFMA_TFLOPS, 3)}
    print(json.dumps({"arch": "resnet_18", "math": "fp16x3", "batch": B, "height": H, "width": W,
                      "steps": a.steps, "warmup": a.warmup, "forward_decode_ms": round(ms, 3),
                      "frames_per_s": round(B / ms * 1e3, 1), "launches": launches,
                      "ceiling": f"dense fp16 MFMA {PEAK_FP16_MFMA_TFLOPS:.0f} TF, 3 products per MAC",
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
