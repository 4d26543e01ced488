#!/usr/bin/env python3
"""Generate tests/golden/resnet_golden*.npz by running the REFERENCE's plain resnet_18.

Same recipe as gen_golden.py (build container only; the reference is imported at run time from a
scratch copy, nothing of it is written here but numbers):

  * models/model_utils.py:25-43   create_model(arch="resnet_18")
  * models/resnet.py:115-234      PoseResNet (ResNet-18, three ConvTranspose2d + BN + ReLU, heads)
  * utils/torch_utils.py:44-45    _sigmoid
  * utils/evaluation_utils.py     _nms / decode

Contents: the state_dict names and shapes; head logits of the small cases (weights
synthetic_state_dict(spec, 0), inputs hash_uniform(seed, 7, .)); for the 64 x 64 case the three
deconv stage outputs after ReLU (forward hooks on deconv_layers[2], [5], [8]); and one 608 x 608
frame end to end (synthetic cloud 1 -> reference BEV -> forward -> _sigmoid -> decode(K=50)):
4,096 sampled logits per head, the (1, 50, 10) detections, the top-51 peak scores.  The 608 x 608
frame's weight seed is the first in 0, 1, 2, ... whose smallest top-51 gap is >= MIN_GAP (asserted
here, on the reference alone; the seed is stored).  MIN_GAP = 5e-5 is the smallest gap that makes the
ranking unambiguous for ANY forward inside the parity bound |d logit| <= 1e-4 max(1, |logit|): the
sigmoid's slope is <= 1/4 (and slope x |logit| <= 0.224), so a score moves by <= 2.5e-5 and two scores
can change order only if they are closer than 5e-5.  (51 scores spread over ~0.15 have a mean gap of
3e-3 and a typical smallest gap of ~5e-5: a 1e-3 floor is met by no seed — 0..63 give 0 .. 6.3e-5.)

Usage:  python tests/golden/gen_resnet_golden.py [--out tests/golden]
"""

from __future__ import annotations

import argparse
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (the import recipe, HEADS, BOUNDARY; puts sfa_hip on the path)
import golden_io  # noqa: E402
from sfa_hip import synthetic  # noqa: E402

HEADS = gg.HEADS
# case -> (B, H, W, input seed); 32 x 32: layer4 is 1 x 1, every deconv neighbour is out of range
CASES = {"b2_96": (2, 96, 96, 31), "b1_160x128": (1, 160, 128, 32), "b3_32": (3, 32, 32, 33),
         "b1_64": (1, 64, 64, 34)}
STAGE_CASE = "b1_64"
MIN_GAP = 5e-5
MAX_SEEDS = 64


def _ref_model(ref, seed):
    import torch
    cfg = gg._Cfg(arch="resnet_18", heads=dict(HEADS), head_conv=64, imagenet_pretrained=False)
    model = gg._quiet(ref["model_utils"].create_model, cfg)
    spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    sd = synthetic.synthetic_state_dict(spec, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.eval()
    return model, spec


def gen(ref, out):
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    model, spec = _ref_model(ref, 0)
    res = {"state_names": np.array([k for k, _ in spec]),
           "state_shapes": np.array([list(s) + [0] * (4 - len(s)) for _, s in spec], dtype=np.int64)}
    with torch.no_grad():
        for case, (B, H, W, seed) in CASES.items():
            x = synthetic.hash_uniform(seed, 7, B * 3 * H * W).astype(np.float32).reshape(B, 3, H, W)
            stages, hooks = [], []
            if case == STAGE_CASE:
                for i in (2, 5, 8):
                    hooks.append(model.deconv_layers[i].register_forward_hook(
                        lambda m, a, o: stages.append(o.detach().numpy().copy())))
            outs = model(torch.from_numpy(x))
            for h in hooks:
                h.remove()
            res[f"{case}/shape"] = np.array([B, H, W])
            assert list(outs) == list(HEADS)
            for h in HEADS:
                res[f"{case}/{h}"] = outs[h].numpy().copy()
            for i, s in enumerate(stages):
                res[f"{case}/deconv{i + 1}"] = s  # NCHW
            print(f"resnet {case}: ok", [float(np.abs(res[f'{case}/{h}']).max()) for h in HEADS])
        cloud = synthetic.synthetic_point_cloud(1)
        bev = ref["bev"].makeBEVMap(ref["data"].get_filtered_lidar(cloud.copy(), gg.BOUNDARY), gg.BOUNDARY)
        x = torch.from_numpy(bev[None]).float()
        rng = np.random.default_rng(1234)
        ys, xs = rng.integers(0, 152, 4096), rng.integers(0, 152, 4096)
        for seed in range(MAX_SEEDS):
            model, _ = _ref_model(ref, seed)
            outs = model(x)
            raw = {h: outs[h].numpy().copy() for h in HEADS}  # _sigmoid is in-place
            hm = ref["tu"]._sigmoid(outs["hm_cen"])
            off = ref["tu"]._sigmoid(outs["cen_offset"])
            top, gap = gg._frame_top51(ref, hm)
            print(f"e2e weight seed {seed}: min top-51 gap {gap[0]:.3g}, top score {top[0][0]:.6f}")
            if gap[0] >= MIN_GAP:
                break
        else:
            raise SystemExit(f"no weight seed below {MAX_SEEDS} gives a top-51 gap >= {MIN_GAP}")
        assert gap[0] >= MIN_GAP
        res["e2e/weight_seed"] = np.array(seed)
        res["e2e/sample_yx"] = np.stack([ys, xs]).astype(np.int32)
        for h in HEADS:
            res[f"e2e/{h}/samples"] = raw[h][0][:, ys, xs]
        res["e2e/dets"] = ref["ev"].decode(hm, off, outs["direction"], outs["z_coor"], outs["dim"], K=50).numpy()
        res["e2e/top51"] = top[0]
        res["e2e/min_gap"] = gap
    golden_io.save(out, "resnet_golden", res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    if not os.path.isdir(gg.REF):
        sys.exit("reference not present: fixtures are generated in the build container only")
    ref = gg._import_reference()
    try:
        gen(ref, a.out)
    finally:
        shutil.rmtree(ref["scratch"], ignore_errors=True)


if __name__ == "__main__":
    main()
