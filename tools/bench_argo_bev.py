"""Timing of the Argoverse BEV voxeliser (sfa_argo_bev_voxelize; makeBVFeature of argoverse_test2.py:198-257),
which bench.py (fixed on the KITTI detector) does not cover.

    python tools/bench_argo_bev.py [--batch 16] [--points 100000] [--steps 50] [--warmup 10]

`batch` resident synthetic sweeps of `points` points (synthetic.synthetic_argoverse_sweep, seeds 1..batch) are
voxelised at 800 x 800 (+-40 m, 0.1 m) by one call captured in a HIP graph: `warmup` untimed replays, then
`steps` replays each between its own pair of events; the median per call in us.  Algorithmic bytes per
frame = N * 16 B read + 3 * H * W * 4 B written; their rate over the 8 TB/s HBM peak is the fraction of the
memory roof (the kernels are memory / atomic bound: no arithmetic to speak of).  The same method times the
NHWC4 layout, the atomic path, and — for context, same process — the KITTI voxeliser on `batch`
synthetic KITTI sweeps at 608 x 608.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"))

HBM_PEAK_TBS = 8.0  # MI355X HBM3E


def algorithmic_bytes(n_points_total, batch, H, W):
    return n_points_total * 16 + batch * 3 * H * W * 4


def time_graph(torch, call, steps, warmup):
    """Median / min us of `steps` replays of the graph of `call` after `warmup` untimed ones."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(warmup):
        g.replay()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        g.replay()
        e1.record()
    torch.cuda.synchronize()
    us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    return statistics.median(us), min(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import numpy as np
    import torch
    from sfa_hip import _lib, runtime, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_argo_bev: no GPU visible (a time is measured on the GPU or not at all)")
    dev = torch.device("cuda", 0)
    B = a.batch
    clouds = [synthetic.synthetic_argoverse_sweep(s, a.points) for s in range(1, B + 1)]
    offs = np.cumsum([0] + [c.shape[0] for c in clouds])
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    vox = runtime.ArgoBevVoxelizer(dev, runtime.ARGO_BOUNDARY, runtime.ARGO_DISCRETIZATION, B)
    H, W = vox.H, vox.W
    nbytes = algorithmic_bytes(int(offs[-1]), B, H, W)
    res = {}
    for name, layout, atomic in (("record_nchw3", _lib.BEV_NCHW3_F32, False), ("record_nhwc4", _lib.BEV_NHWC4_F32, False),
                                 ("atomic_nchw3", _lib.BEV_NCHW3_F32, True)):
        out = torch.empty(vox.out_shape(B, layout), dtype=torch.float32, device=dev)
        med, mn = time_graph(torch, lambda: vox(pts, offs, layout=layout, out=out, force_atomic=atomic), a.steps,
                             a.warmup)
        wr = B * H * W * 4 * (4 if layout == _lib.BEV_NHWC4_F32 else 3)
        res[name] = {"median_us": round(med, 1), "min_us": round(mn, 1),
                     "algorithmic_tbs": round((int(offs[-1]) * 16 + wr) / (med * 1e-6) / 1e12, 3),
                     "fraction_of_hbm": round((int(offs[-1]) * 16 + wr) / (med * 1e-6) / 1e12 / HBM_PEAK_TBS, 3)}
    # context: the KITTI voxeliser, same process, same method, its own sweeps and map
    kc = [synthetic.synthetic_point_cloud(s) for s in range(1, B + 1)]
    koffs = np.cumsum([0] + [c.shape[0] for c in kc])
    kpts = torch.from_numpy(np.concatenate(kc)).to(dev)
    kvox = runtime.BevVoxelizer(dev, B)
    kout = torch.empty((B, 3, 608, 608), dtype=torch.float32, device=dev)
    kmed, kmin = time_graph(torch, lambda: kvox(kpts, koffs, layout=_lib.BEV_NCHW3_F32, out=kout), a.steps, a.warmup)
    kbytes = algorithmic_bytes(int(koffs[-1]), B, 608, 608)
    res["kitti_608_nchw3"] = {"median_us": round(kmed, 1), "min_us": round(kmin, 1), "points": int(koffs[-1]),
                              "algorithmic_tbs": round(kbytes / (kmed * 1e-6) / 1e12, 3),
                              "fraction_of_hbm": round(kbytes / (kmed * 1e-6) / 1e12 / HBM_PEAK_TBS, 3)}
    print(json.dumps({"bench": "argo_bev", "batch": B, "points_per_sweep": a.points, "height": H, "width": W,
                      "steps": a.steps, "warmup": a.warmup, "algorithmic_bytes": nbytes,
                      "hbm_peak_tbs": HBM_PEAK_TBS, "results": res, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
