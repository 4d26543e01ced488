#!/usr/bin/env python3
"""The reference's validation loop (train.py:250-275 validate) on the HIP path: targets built on the GPU from
the labels (sfa_build_targets), the forward, the loss (sfa_compute_loss), the AverageMeter average of
total_loss over the frames, one JSON line.

  tools/validate.py --synthetic 16                     synthetic weights, frames and labels (no data set)
  tools/validate.py --dataset_dir D --pretrained_path P   KITTI val split through create_val_dataloader
  --math fp16      also runs SFA_MATH_FP16 on the same frames and reports its loss next to fp16x3's
  --timing         median microseconds of target build + loss for 16 frames on a captured HIP graph
  --timing --grad  also targets + loss + gradient (sfa_compute_loss_grad) on one graph, then bench.py
  --timing --grad --kfpn   also that graph with the KFPN gradient (sfa_kfpn_combine_grad) behind the loss gradient
  --timing --grad --kfpn --heads   also that graph with the head parameter gradients (sfa_model_heads_grad) of one,
                           two and all three KFPN levels behind the KFPN gradient
  --timing --grad --kfpn --heads --dgrad   also that last graph with the heads' input gradient
                           (sfa_model_heads_input_grad) of one, two and all three levels added
  --timing --grad --kfpn --heads --dgrad --neck   also that last graph with the FPN neck's gradient
                           (sfa_model_neck_grad: the four maps' and the six parameters' gradients) added

The loop is evaluation only (the gradient at the heads is only timed).  With a data set, the labels of a batch are read with the
data set's own helpers (get_label, camera_to_lidar_box, filter_labels: a reference tree on sys.path or in
SFA_REFERENCE_ROOT serves get_label), the maps come from the drop-in loader.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SFA_ROOT = os.path.join(REPO, "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa")
for p in (REPO, SFA_ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from sfa_hip import _lib, runtime, synthetic  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


class AverageMeter:
    """utils/misc.py:20-41, the part validate uses."""

    def __init__(self):
        self.sum, self.count = 0.0, 0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n

    @property
    def avg(self):
        return self.sum / max(self.count, 1)


def make_model(args, device):
    from models.model_utils import create_model
    model = create_model(Cfg(arch=args.arch, heads=dict(runtime.DEFAULT_HEADS), head_conv=64,
                             imagenet_pretrained=False))
    if args.pretrained_path:
        model.load_state_dict(torch.load(args.pretrained_path, map_location="cpu"))
    else:
        spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        sd = synthetic.synthetic_state_dict(spec, args.seed)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(device).eval()


def synthetic_batches(args, device):
    """(maps (B, 3, H, W) on the device, labels (N, 8), offsets, hflipped) per batch."""
    H = W = args.input_size
    for start in range(0, args.synthetic, args.batch_size):
        B = min(args.batch_size, args.synthetic - start)
        x = synthetic.synthetic_bev(B, H, W, seed=args.seed + start)
        labels, offsets = synthetic.synthetic_labels(B, seed=args.seed + start)
        yield torch.from_numpy(x).to(device), labels, offsets, [False] * B


def dataset_batches(args, device):
    import config.kitti_config as cnf
    from data_process import transformation
    from data_process.kitti_data_utils import filter_labels
    from data_process.kitti_dataloader import create_val_dataloader
    H = W = args.input_size
    configs = Cfg(dataset_dir=args.dataset_dir, input_size=(H, W), hm_size=(H // 4, W // 4), num_classes=3,
                  max_objects=args.max_objects, num_samples=args.num_samples, distributed=False,
                  batch_size=args.batch_size, num_workers=args.num_workers, pin_memory=True)
    loader = create_val_dataloader(configs)
    ds = loader.dataset
    index = 0
    for metadatas, bev_maps, _targets in loader:  # the val loader is not shuffled: batch i = the next B samples
        B = int(bev_maps.shape[0])
        rows, offsets = [], [0]
        for i in range(index, index + B):
            sample_id = int(ds.sample_id_list[i])
            labels, has = ds.get_label(sample_id)
            if has:
                calib = ds.get_calib(sample_id)
                labels[:, 1:] = transformation.camera_to_lidar_box(labels[:, 1:], calib.V2C, calib.R0, calib.P2)
            labels = filter_labels(labels, cnf.boundary)
            rows.append(np.asarray(labels, np.float32).reshape(-1, 8))
            offsets.append(offsets[-1] + rows[-1].shape[0])
        index += B
        flips = [bool(f) for f in metadatas["hflipped"]]
        yield bev_maps.to(device).float(), np.concatenate(rows), np.int64(offsets), flips


def evaluate(model, batches, args, device):
    from losses.losses import Compute_Loss
    criterion = Compute_Loss(device)
    hm = args.input_size // 4
    builder = runtime.TargetBuilder(device, runtime.DEFAULT_BOUNDARY, (hm, hm), 3, args.max_objects)
    losses, parts, frames = AverageMeter(), {}, 0
    with torch.no_grad():
        for x, labels, offsets, flips in batches:
            B = int(x.shape[0])
            targets = builder(labels, [int(o) for o in offsets], flips)
            outputs = model(x)
            total, stats = criterion(outputs, targets)
            losses.update(stats["total_loss"], B)  # train.py:268 reduced_loss.item(), batch_size
            for k, v in stats.items():
                parts[k] = parts.get(k, 0.0) + v * B
            frames += B
    return losses.avg, {k: v / max(frames, 1) for k, v in parts.items()}, frames


def timing(device, args, frames=16, reps=50, grad=False, kfpn=False, heads_levels=0, engine=None, dgrad_levels=0,
           neck=False):
    """Median microseconds of sfa_build_targets + sfa_compute_loss (with ``grad`` also sfa_compute_loss_grad, with
    ``kfpn`` also sfa_kfpn_combine_grad from the head gradients to the 15 per-level maps, level 0 at half
    resolution; with ``heads_levels`` = n also sfa_model_heads_grad of KFPN levels 0 .. n - 1 of ``engine`` from those
    level gradients and a synthetic heads' input; with ``dgrad_levels`` = n also sfa_model_heads_input_grad of levels
    0 .. n - 1 on a synthetic dA of the level's shape: its time does not depend on the values; with ``neck`` also
    sfa_model_neck_grad, all ten outputs, from the three input gradients and synthetic backbone maps) for ``frames``
    frames, one HIP graph."""
    hm = args.input_size // 4
    labels, offsets = synthetic.synthetic_labels(frames, seed=args.seed)
    builder = runtime.TargetBuilder(device, runtime.DEFAULT_BOUNDARY, (hm, hm), 3, args.max_objects)
    ev = runtime.LossEvaluator(device)
    d_labels = torch.from_numpy(labels).to(device)
    d_offsets = torch.from_numpy(offsets).to(device)
    outs = {h: torch.from_numpy(synthetic.synthetic_logits((frames, c, hm, hm), args.seed, 60 + i)).to(device)
            for i, (h, c) in enumerate(runtime.DEFAULT_HEADS.items())}
    tg = builder.alloc(frames)
    grads = {h: torch.empty_like(t) for h, t in outs.items()}
    if kfpn:
        sizes = (hm // 2, hm, hm)  # level 0 at half resolution
        levels = {h: [torch.from_numpy(synthetic.synthetic_logits((frames, c, n, n), args.seed, 80 + 3 * i + l)).to(device)
                      for l, n in enumerate(sizes)]
                  for i, (h, c) in enumerate(runtime.DEFAULT_HEADS.items())}
        level_grads = {h: [torch.empty_like(t) for t in lv] for h, lv in levels.items()}

    hg = []
    for level in range(heads_levels):
        n, cin = sizes[level], _lib.HEADS_LEVEL_CIN[level]
        x = torch.from_numpy(np.abs(synthetic.synthetic_logits((frames, n, n, cin), args.seed, 120 + level))).to(device)
        out = {h: [torch.empty(s, dtype=torch.float32, device=device)
                   for s in ((64, cin, 3, 3), (64,), (c, 64, 1, 1), (c,))] for h, c in runtime.DEFAULT_HEADS.items()}
        ws = torch.empty(engine.heads_grad_workspace_bytes(level, frames, n, n), dtype=torch.uint8, device=device)
        hg.append((level, x, {h: lv[level] for h, lv in level_grads.items()}, out, ws))

    dg = []
    for level in range(dgrad_levels):
        n = sizes[level]
        dA = torch.from_numpy(synthetic.synthetic_logits((frames, n, n, 64 * len(runtime.DEFAULT_HEADS)), args.seed,
                                                         140 + level)).to(device)
        dg.append((level, dA, torch.empty((frames, n, n, _lib.HEADS_LEVEL_CIN[level]), dtype=torch.float32, device=device)))

    nk = None
    if neck:
        h4 = args.input_size // 32
        shapes = engine._neck_shapes(frames, h4, h4)
        maps = [torch.from_numpy(synthetic.synthetic_logits(sh, args.seed, 160 + i)).to(device)
                for i, sh in enumerate(shapes[:6])]
        mk = lambda shs: [torch.empty(sh, dtype=torch.float32, device=device) for sh in shs]  # noqa: E731
        nk = (maps[:4], maps[4:6], (mk(shapes[:4]), mk(_lib.NECK_PARAM_SHAPES)),
              torch.empty(engine.neck_grad_workspace_bytes(frames, h4, h4), dtype=torch.uint8, device=device))

    def step():
        builder(d_labels, d_offsets, None, out=tg, verify=False)
        ev(outs, tg, apply_sigmoid=True, verify=False)
        if grad:
            ev.grad(outs, tg, apply_sigmoid=True, verify=False, out=grads)
        if kfpn:
            runtime.kfpn_combine_grad(levels, grads, level0_half=True, out=level_grads)
        for level, x, g, out, ws in hg:
            engine.heads_param_grad(level, x, g, out=out, workspace=ws)
        for level, dA, gx in dg:
            engine.heads_input_grad(level, dA, out=gx)
        if nk:
            engine.neck_grad(*(gx for _, _, gx in dg), layers=nk[0], ups=nk[1], out=nk[2], workspace=nk[3])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return {"frames": frames, "reps": reps, "median_us": float(np.median(times)), "min_us": float(np.min(times))}


def run_bench():
    """``python bench.py`` in a child process, after this one's GPU work: its JSON line (the inference path)."""
    import subprocess
    torch.cuda.synchronize()
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")], capture_output=True, text=True, cwd=REPO)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not lines:
        return {"error": f"bench.py exited with {out.returncode}", "stderr": out.stderr[-500:]}
    return json.loads(lines[-1])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arch", default="fpn_resnet_18", choices=["fpn_resnet_18", "resnet_18"])
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic frames instead of a data set")
    ap.add_argument("--dataset_dir", default=None)
    ap.add_argument("--pretrained_path", default=None)
    ap.add_argument("--num_samples", type=int, default=None)
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--num_workers", type=int, default=2)
    ap.add_argument("--input_size", type=int, default=608)
    ap.add_argument("--max_objects", type=int, default=50)
    ap.add_argument("--math", default=None, choices=["fp16"], help="also report the loss under SFA_MATH_FP16")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--grad", action="store_true",
                    help="with --timing: also time targets + loss + gradient on one graph, then run bench.py")
    ap.add_argument("--kfpn", action="store_true",
                    help="with --timing --grad: also time that graph with the KFPN gradient added (one run, no threshold)")
    ap.add_argument("--heads", action="store_true",
                    help="with --timing --grad --kfpn: also time that graph with the head parameter gradients of KFPN "
                         "levels 0, 0-1 and 0-2 added (one run, no threshold)")
    ap.add_argument("--dgrad", action="store_true",
                    help="with --timing --grad --kfpn --heads: also time the three-level graph with the heads' input "
                         "gradient of levels 0, 0-1 and 0-2 added (one run, no threshold)")
    ap.add_argument("--neck", action="store_true",
                    help="with --timing --grad --kfpn --heads --dgrad: also time the last graph with the FPN neck's "
                         "gradient added (one run, no threshold)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gpu_idx", type=int, default=0)
    args = ap.parse_args(argv)
    if not args.synthetic and not args.dataset_dir:
        ap.error("give --synthetic N or --dataset_dir")
    if args.input_size % 32:
        ap.error("--input_size must be a multiple of 32")
    device = torch.device("cuda", args.gpu_idx)
    model = make_model(args, device)
    source = synthetic_batches if args.synthetic else dataset_batches
    t0 = time.time()
    avg, parts, frames = evaluate(model, source(args, device), args, device)
    result = {"arch": args.arch, "frames": frames, "math": "fp16x3", "val_loss": avg, "loss_stats": parts,
              "seconds": round(time.time() - t0, 3)}
    if args.math == "fp16":
        model.set_math("fp16")
        avg16, parts16, _ = evaluate(model, source(args, device), args, device)
        result["fp16"] = {"val_loss": avg16, "loss_stats": parts16, "delta_vs_fp16x3": avg16 - avg}
    if args.timing:
        result["targets_plus_loss_graph"] = timing(device, args)
        if args.grad:
            result["targets_plus_loss_plus_grad_graph"] = timing(device, args, grad=True)
            if args.kfpn:
                result["targets_plus_loss_plus_grad_plus_kfpn_grad_graph"] = timing(device, args, grad=True, kfpn=True)
                if args.heads:
                    if args.arch != "fpn_resnet_18":
                        ap.error("--heads needs the KFPN model (fpn_resnet_18)")
                    eng = model._engine(device)
                    for n in (1, 2, 3):
                        result[f"plus_heads_grad_levels_0_to_{n - 1}_graph"] = timing(
                            device, args, grad=True, kfpn=True, heads_levels=n, engine=eng)
                    if args.dgrad:
                        for n in (1, 2, 3):
                            result[f"plus_heads_input_grad_levels_0_to_{n - 1}_graph"] = timing(
                                device, args, grad=True, kfpn=True, heads_levels=3, engine=eng, dgrad_levels=n)
                        if args.neck:
                            result["plus_neck_grad_graph"] = timing(
                                device, args, grad=True, kfpn=True, heads_levels=3, engine=eng, dgrad_levels=3, neck=True)
            result["bench"] = run_bench()
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
