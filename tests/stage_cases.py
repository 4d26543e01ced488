"""Inputs, stage plumbing and error metrics of the stage-by-stage forward parity tests
(tests/test_stage_premises.py on the CPU, tests/test_gpu_model_stages.py on the GPU).

A forward is cut into eleven stages, each judged on exactly the inputs it was given:

  layer1              x                        oracle.model_oracle.stage_layer1
  layer2..4           layer1..3                stage_layer
  up_level2..4        (layer4, layer3), (up_level2, layer2), (up_level3, layer1)      stage_up
  heads0..2/<head>    up_level2..4             stage_heads
  out/<head>          heads0..2/<head>         stage_combine

Maps travel as one flat dict {name: (B, C, h, w) torch tensor} with those names plus "x".
"""
import math

import numpy as np
import torch

from oracle import model_oracle as mo
from sfa_hip import synthetic

# exact in f32; three different binary exponents and an empty frame (an empty sweep's BEV map)
FACTORS = (1.0, 2.0 ** -6, 2.0 ** 9, 0.0)
# the maps a later convolution reads, i.e. the ones fp16x3 scales per frame by a power of two
SCALED_MAPS = ("layer1", "layer2", "layer3", "layer4", "up_level2", "up_level3", "up_level4")
GATE = 1e-5  # forward per kernel vs torch CPU on identical inputs


def mixed_batch(B, H, W, seed):
    """synthetic_bev frames times FACTORS[b % 4]."""
    x = synthetic.synthetic_bev(B, H, W, seed=seed)
    f = np.float32([FACTORS[b % len(FACTORS)] for b in range(B)])
    return x * f[:, None, None, None]


def sparse_batch(B, H, W, seed):
    """BEV-like: nine cells in ten empty."""
    x = synthetic.synthetic_bev(B, H, W, seed=seed).copy()
    x[x < 0.9] = 0
    return x


def _f64(a):
    return a.detach().cpu().to(torch.float64).numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)


def err_elem(got, ref):
    """max |d| / max(1, |ref|) over all elements — the SURVEY metric, for natural amplitudes."""
    got, ref = _f64(got), _f64(ref)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def err_frame(got, ref):
    """Per frame b: max |d_b| / max(1, max |ref_b|) — for frames whose activations reach 2e3, where the
    elementwise measure against elements near 1 is dominated by cancellation."""
    got, ref = _f64(got), _f64(ref)
    B = ref.shape[0]
    d = np.abs(got - ref).reshape(B, -1).max(1)
    return d / np.maximum(1.0, np.abs(ref).reshape(B, -1).max(1))


def worst_index(got, ref, frame=None):
    """Index (b, c, y, x) of the largest |d| (within `frame` if given)."""
    d = np.abs(_f64(got) - _f64(ref))
    if frame is not None:
        return (frame,) + tuple(int(i) for i in np.unravel_index(int(np.argmax(d[frame])), d.shape[1:]))
    return tuple(int(i) for i in np.unravel_index(int(np.argmax(d)), d.shape))


def frame_exponents(t):
    """floor(log2 max |t_b|) per frame (None for an all-zero frame): what picks the fp16x3 scale."""
    mx = np.abs(_f64(t)).reshape(t.shape[0], -1).max(1)
    return [math.frexp(float(m))[1] - 1 if m > 0 else None for m in mx]


def stage_names(heads):
    names = ["layer1", "layer2", "layer3", "layer4", "up_level2", "up_level3", "up_level4"]
    names += [f"heads{f}/{h}" for f in range(3) for h in heads]
    return names + [f"out/{h}" for h in heads]


def run_stages(sd, maps, heads, chain=False, only=None):
    """Every stage's oracle output, {name: tensor}, in sd's dtype.  chain=False: each stage reads ITS inputs
    from `maps` (cast to the dtype); chain=True: only maps["x"] is read and every stage reads the oracle's
    own previous outputs (a whole forward).  only: the stage groups to evaluate ("layer1", ..., "up_level2",
    ..., "heads0", ..., "out"); the default is all of them."""
    dt = sd["conv1.weight"].dtype
    o = {}

    def want(group):
        return only is None or group in only

    def src(name):
        t = o[name] if chain and name != "x" else maps[name]
        return t.detach().cpu().to(dt)

    if want("layer1"):
        o["layer1"] = mo.stage_layer1(sd, src("x"))
    for k in (2, 3, 4):
        if want(f"layer{k}"):
            o[f"layer{k}"] = mo.stage_layer(sd, k, src(f"layer{k - 1}"))
    if want("up_level2"):
        o["up_level2"] = mo.stage_up(sd, 0, src("layer4"), src("layer3"))
    if want("up_level3"):
        o["up_level3"] = mo.stage_up(sd, 1, src("up_level2"), src("layer2"))
    if want("up_level4"):
        o["up_level4"] = mo.stage_up(sd, 2, src("up_level3"), src("layer1"))
    for f in range(3):
        if want(f"heads{f}"):
            for h, t in mo.stage_heads(sd, f, src(f"up_level{f + 2}"), heads).items():
                o[f"heads{f}/{h}"] = t
    if want("out"):
        hm_h, hm_w = maps["x"].shape[2] // 4, maps["x"].shape[3] // 4
        for h in heads:
            o[f"out/{h}"] = mo.stage_combine([src(f"heads{f}/{h}") for f in range(3)], hm_h, hm_w)
    return o


def compare(got, ref, heads, per_frame):
    """[(stage, frame or None, error, worst index)] for every stage (and frame, if per_frame)."""
    rows = []
    for name in stage_names(heads):
        if name not in ref:
            continue
        if per_frame:
            e = err_frame(got[name], ref[name])
            rows += [(name, b, float(e[b]), worst_index(got[name], ref[name], b)) for b in range(len(e))]
        else:
            rows.append((name, None, err_elem(got[name], ref[name]), worst_index(got[name], ref[name])))
    return rows


def format_rows(title, rows, heads):
    """One table line per stage: the worst error over its heads / frames."""
    worst = {}
    for name, b, e, idx in rows:
        key = name.split("/")[0]
        if key not in worst or e > worst[key][0]:
            worst[key] = (e, name, b, idx)
    lines = [title]
    for key, (e, name, b, idx) in worst.items():
        where = name + ("" if b is None else f" frame {b}")
        lines.append(f"  {key:10s} {e:9.3g}   worst: {where} at {idx}")
    return "\n".join(lines)


def failures(rows, gate=GATE):
    return [f"{name}{'' if b is None else f' frame {b}'}: {e:.3g} > {gate:g} at {idx}"
            for name, b, e, idx in rows if not e <= gate]
