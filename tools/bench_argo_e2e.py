"""Timing of the Argoverse scripts' configuration end to end, which bench.py (fixed on the KITTI
detector) does not cover: BEV (makeBVFeature, 800 x 800) -> KFPN forward -> decode (200 x 200 heat map,
the tiled form) on one HIP graph.

    python tools/bench_argo_e2e.py [--batch 16] [--points 100000] [--steps 50] [--warmup 10]

`batch` resident synthetic sweeps of `points` points (synthetic.synthetic_argoverse_sweep, seeds
1..batch); the whole step and each stage on its own are captured in a graph, `warmup` untimed replays,
then `steps` replays each between its own pair of events (tools/bench_argo_bev.time_graph); medians in
us.  Beside it, in the same process and by the same method: the decode alone at (batch, 3, 200, 200)
(tiled) and at (batch, 3, 152, 152) (the band form), K = 50, on random logits.  `decode_yardstick_us`
is the band form's time scaled by the cell ratio 40000 / 23104.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--K", type=int, default=50)
    a = ap.parse_args()
    import torch
    from bench_argo_bev import time_graph
    from sfa_hip import _lib, runtime, synthetic
    if not torch.cuda.is_available():
        sys.exit("bench_argo_e2e: no GPU visible (a time is measured on the GPU or not at all)")
    dev = torch.device("cuda", 0)
    B, K = a.batch, a.K
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    packed = runtime.pack_state_dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), 0), arch)
    eng = runtime.KfpnEngine(arch, packed, dev)
    clouds = [synthetic.synthetic_argoverse_sweep(s, a.points) for s in range(1, B + 1)]
    pipe = runtime.DetectorPipeline(eng, B, 800, 800, K=K, with_bev=True, max_points=sum(c.shape[0] for c in clouds),
                                    bev="argoverse", boundary=runtime.ARGO_BOUNDARY,
                                    discretization=runtime.ARGO_DISCRETIZATION)
    pipe.set_points(clouds)
    st = lambda: _lib.stream_ptr(dev)
    o = pipe.outs
    dec = runtime.Decoder()

    def bev():
        pipe.vox(pipe.points, pipe.offsets, layout=pipe.bev_fmt, out=pipe.bev, stream=st())

    def forward():
        eng.forward_into(pipe.bev, pipe.outs, pipe.in_fmt, pipe.ws, st())

    def decode():
        dec(o["hm_cen"], o["cen_offset"], o["direction"], o["z_coor"], o["dim"], K=K, apply_sigmoid=True,
            out=pipe.dets, stream=st(), workspace=pipe.dec_ws)

    res = {}
    for name, call in (("e2e", lambda: pipe.run(_eager=True)), ("bev", bev), ("forward", forward), ("decode", decode)):
        med, mn = time_graph(torch, call, a.steps, a.warmup)
        res[name] = {"median_us": round(med, 1), "min_us": round(mn, 1)}
    res["e2e"]["frames_per_s"] = round(B / (res["e2e"]["median_us"] * 1e-6), 1)

    # decode alone: the tiled form at 200 x 200 beside the band form at 152 x 152, random logits
    alone = {}
    for side in (200, 152):
        g = torch.Generator(device=dev).manual_seed(side)
        maps = {k: torch.randn((B, c, side, side), generator=g, device=dev) for k, c in
                (("hm", 3), ("off", 2), ("dir", 2), ("z", 1), ("dim", 3))}
        out = torch.empty((B, K, 10), dtype=torch.float32, device=dev)
        ws = torch.empty(dec.workspace_bytes(B, 3, K, side, side), dtype=torch.uint8, device=dev)
        med, mn = time_graph(torch, lambda: dec(maps["hm"], maps["off"], maps["dir"], maps["z"], maps["dim"], K=K,
                                                apply_sigmoid=True, out=out, stream=st(), workspace=ws),
                             a.steps, a.warmup)
        alone[f"decode_{side}"] = {"median_us": round(med, 1), "min_us": round(mn, 1)}
    yard = alone["decode_152"]["median_us"] * 40000 / 23104
    alone["decode_yardstick_us"] = round(yard, 1)
    alone["decode_200_over_yardstick"] = round(alone["decode_200"]["median_us"] / yard, 3)
    print(json.dumps({"bench": "argo_e2e", "batch": B, "points_per_sweep": a.points, "height": 800, "width": 800,
                      "K": K, "steps": a.steps, "warmup": a.warmup, "results": res, "decode_alone": alone,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
