"""Head sets other than the production one: the sets, their models, the premises of their parity tests
(tests/test_headsets_host.py on the CPU, tests/test_gpu_headsets.py on the GPU) and the corruptions the
checker must notice.

The descriptor admits 1..8 heads of 1..4 channels (include/sfa_hip.h sfa_arch).  Head sets are written in
INSERTION order, the order of the forward's output dict and of the channel-planar level blocks (hoff,
KfpnOut::off); the state dict registers the heads in sorted() order.  In "two", "five_wide" and "six" the two
orders differ, and heads that swap places have different widths, so a mix-up changes a shape or an offset.

  one         N =  64   one column tile, one output channel
  two         N = 128   unsorted order; a 4-channel head off the production kernel
  three       N = 192   the set of test_gpu_math_fp16.test_three_heads_fall_back
  five_wide   N = 320   the production kernel and its W image with ch = 4 (output o = 3 of the packed head
                        epilogue, lanes 48..63, the fourth w1 / b1 row); offsets 0, 4, 5, 9, 11, 15 channels
  five_ones   N = 320   the production kernel with ch = 1 in every head
  six         N = 384   N % 128 == 0, yet the head route
  eight_full  N = 512   SFA_MAX_HEADS x 4 channels = 32, grid.y = 8
"""
import numpy as np
import torch
import torch.nn.functional as F

import stage_cases as sc
from oracle import model_oracle as mo
from sfa_hip import _lib, synthetic

SETS = {
    "one": {"hm_cen": 1},
    "two": {"z_coor": 1, "cen_offset": 4},
    "three": {"hm_cen": 3, "cen_offset": 2, "z_coor": 1},
    "five_wide": {"hm_cen": 4, "dim": 1, "direction": 4, "cen_offset": 2, "z_coor": 4},
    "five_ones": {"hm_cen": 1, "cen_offset": 1, "direction": 1, "z_coor": 1, "dim": 1},
    "six": {"hm_cen": 3, "cen_offset": 2, "direction": 2, "z_coor": 1, "dim": 3, "aux": 4},
    "eight_full": {"hm_cen": 4, "cen_offset": 4, "direction": 4, "z_coor": 4, "dim": 4, "yaw": 4, "vel": 4, "attr": 4},
}
UNSORTED = ("two", "five_wide", "six")
WEIGHT_SEED = 5  # test_gpu_math_fp16.make_model's seed for synthetic weights
INPUT_SEED = 83
BATCHES = {
    # level maps 4x6, 8x12, 16x24: M = 72 (under one 256-row tile), 288 (a tile + 32 rows), 1152 (4.5 tiles)
    "3x64x96": lambda: sc.mixed_batch(3, 64, 96, INPUT_SEED),
    # M = 20, 80, 320: one tile spans all five frames
    "5x32x32": lambda: sc.mixed_batch(5, 32, 32, INPUT_SEED),
}
GROUPS = ("heads0", "heads1", "heads2", "out")
DISTINCT = 100 * sc.GATE  # two channels of a set differ by at least this much
# the reference fixture (tests/golden/gen_headsets_golden.py): (arch, set) and its input
FIXTURE_CASES = (("fpn_resnet_18", "one"), ("fpn_resnet_18", "five_wide"), ("fpn_resnet_18", "eight_full"),
                 ("resnet_18", "five_wide"))
FIXTURE_INPUT = (2, 64, 96, 43)  # B, H, W, hash_uniform seed


class Cfg(dict):
    __getattr__ = dict.__getitem__


def fixture_input():
    B, H, W, seed = FIXTURE_INPUT
    return synthetic.hash_uniform(seed, 7, B * 3 * H * W).astype(np.float32).reshape(B, 3, H, W)


def make_arch(heads, arch="fpn_resnet_18"):
    return _lib.make_arch(dict(heads), backbone=_lib.BACKBONE_DECONV if arch == "resnet_18" else None)


def head_prefixes(heads, arch="fpn_resnet_18"):
    """[(head, state-dict prefix)] of every head module, in forward order within a level."""
    if arch == "resnet_18":
        return [(h, h) for h in heads]
    return [(h, f"fpn{f}_{h}") for f in range(3) for h in heads]


def condition_biases(sd, heads, arch="fpn_resnet_18"):
    """The bias premises, enforced in place on a numpy state dict: every `.0.bias` and `.2.bias` entry of every
    head nonzero, no two head modules with the same `.2.bias` vector (a kernel that dropped a bias, or read
    another head's, then cannot pass).  synthetic_state_dict draws the biases from U(-0.1, 0.1) per entry name,
    so neither happens with the seeds in use and this changes nothing; where it would, a zero entry k becomes
    0.05 + 0.001 k and a repeated vector gets + 0.01 (its position in the list) — a pure function of the
    state dict, the same in the fixture generator and in the tests.  Returns the number of entries changed."""
    changed = 0
    seen = []
    for i, (_, p) in enumerate(head_prefixes(heads, arch)):
        for leaf in (".0.bias", ".2.bias"):
            b = sd[p + leaf]
            for k in np.flatnonzero(b == 0):
                b[k] = np.float32(0.05 + 0.001 * k)
                changed += 1
        b2 = sd[p + ".2.bias"]
        while any(b2.shape == s.shape and np.array_equal(b2, s) for s in seen):
            b2 += np.float32(0.01 * (i + 1))
            changed += b2.size
        seen.append(b2)
    return changed


def state_dict_np(heads, arch="fpn_resnet_18", seed=WEIGHT_SEED):
    """The synthetic state dict of the set's model, biases conditioned (condition_biases)."""
    sd = synthetic.synthetic_state_dict(_lib.state_layout(make_arch(heads, arch)), seed)
    condition_biases(sd, heads, arch)
    return sd


def make_model(arch, heads, device, seed=WEIGHT_SEED):
    """(model, numpy state dict): create_model's model with the synthetic weights, as
    test_gpu_math_fp16.make_model builds it."""
    from models.model_utils import create_model
    model = create_model(Cfg(arch=arch, heads=dict(heads), head_conv=64, imagenet_pretrained=False))
    sd = state_dict_np(heads, arch, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.to(device).eval(), sd


def head_state_f64(sd, heads, arch="fpn_resnet_18"):
    """The head entries (and conv1.weight, which tells run_stages the dtype) as f64 torch tensors."""
    keys = [p + leaf for _, p in head_prefixes(heads, arch) for leaf in (".0.weight", ".0.bias", ".2.weight", ".2.bias")]
    return mo.state_dict_torch({k: sd[k] for k in ["conv1.weight"] + keys}, torch.float64)


def _math(name):
    return _lib.MATH_NAMES[name]


def gpu_maps(eng, x, heads, math="fp16x3", options=None, frames=None):
    """One forward of x (numpy or device tensor) in an explicit workspace -> the flat stage maps
    (stage_cases) as device tensors, own copies: test_gpu_model_stages.gpu_maps for any head set.
    options: {_lib.OPT_*: value} set before the forward; frames: a slice of the batch to keep."""
    dev = eng.device
    eng.set_math(_math(math))
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    x = (torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x).to(dev).contiguous()
    B, _, H, W = x.shape
    sl = slice(None) if frames is None else frames
    with torch.cuda.device(dev):
        ws = torch.empty(eng.workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
        outs = eng.alloc_outputs(B, H, W)
        eng.forward_into(x, outs, workspace=ws)
        torch.cuda.synchronize()
        v = eng.debug_views(ws, B, H, W)
        maps = {"x": x[sl].clone()}
        for k in sc.SCALED_MAPS:
            maps[k] = v[k][sl].contiguous().clone()
        for h in heads:
            for f in range(3):
                maps[f"heads{f}/{h}"] = v["levels"][h][f][sl].contiguous().clone()
            maps[f"out/{h}"] = outs[h][sl].clone()
        torch.cuda.synchronize()
    return maps


def to_cpu(maps):
    return {k: v.cpu() for k, v in maps.items()}


def assert_layout(maps, heads, B, H, W):
    """Key order and shapes of the output dict and of the per-level maps: insertion order, (B, c, h, w)."""
    outs = [k for k in maps if k.startswith("out/")]
    assert outs == [f"out/{h}" for h in heads], outs
    for h, c in heads.items():
        assert tuple(maps[f"out/{h}"].shape) == (B, c, H // 4, W // 4), (h, tuple(maps[f"out/{h}"].shape))
        for f, d in enumerate((8, 4, 4)):
            assert tuple(maps[f"heads{f}/{h}"].shape) == (B, c, H // d, W // d), (f, h)


def oracle_heads_and_out(sd64, maps, heads):
    """The f64 oracle's per-level head maps on maps["up_level2..4"], and its combine of THOSE: oracle-only
    data for the premises (run_stages without chain reads the combine's inputs from `maps`)."""
    ref = sc.run_stages(sd64, maps, heads, only=GROUPS[:3])
    both = dict(maps)
    both.update(ref)
    ref.update(sc.run_stages(sd64, both, heads, only=("out",)))
    return ref


def hidden(sd64, prefix, inp):
    """conv3x3 + bias -> ReLU of one head module."""
    return F.relu(F.conv2d(inp.to(torch.float64), sd64[prefix + ".0.weight"], sd64[prefix + ".0.bias"], 1, 1))


def assert_weight_premises(sd, heads, arch="fpn_resnet_18"):
    """On the weights: every head bias entry nonzero, no `.2.bias` vector shared."""
    seen = []
    for _, p in head_prefixes(heads, arch):
        for leaf in (".0.bias", ".2.bias"):
            assert np.all(np.asarray(sd[p + leaf]) != 0), p + leaf
        b2 = np.asarray(sd[p + ".2.bias"])
        assert not any(b2.shape == s.shape and np.array_equal(b2, s) for s in seen), p
        seen.append(b2)


def channel_table(ref, heads, group):
    """All channels of one group ("heads0", ..., "out") in forward order: (B, sum c, h, w) f64 numpy."""
    return np.concatenate([ref[f"{group}/{h}"].detach().cpu().to(torch.float64).numpy() for h in heads], axis=1)


def assert_output_premises(ref, heads, what):
    """On oracle outputs ({stage name: tensor}; never on the GPU's): at every level every channel has a nonzero
    range, and any two channels of the set differ by at least DISTINCT, elementwise (stage_cases.err_elem)
    and in some frame of the per-frame metric the GPU test gates on (err_frame): a permuted, shifted or
    duplicated channel is then 100 gates away from passing."""
    for g in GROUPS:
        if f"{g}/{next(iter(heads))}" not in ref:
            continue
        t = channel_table(ref, heads, g)
        rng = t.max(axis=(0, 2, 3)) - t.min(axis=(0, 2, 3))
        assert np.all(rng > 0), (what, g, rng.tolist())
        for i in range(t.shape[1]):
            for j in range(i + 1, t.shape[1]):
                a, b = t[:, i:i + 1], t[:, j:j + 1]
                e = min(sc.err_elem(a, b), sc.err_elem(b, a))
                ef = min(float(sc.err_frame(a, b).max()), float(sc.err_frame(b, a).max()))
                assert e >= DISTINCT and ef >= DISTINCT, (what, g, i, j, e, ef)


def assert_relu_live(sd64, maps, heads, what):
    """Every head's hidden activation has both zero and positive entries, at every level."""
    for f in range(3):
        for h in heads:
            hd = hidden(sd64, f"fpn{f}_{h}", maps[f"up_level{f + 2}"].detach().cpu())
            assert bool((hd == 0).any()) and bool((hd > 0).any()), (what, f, h)


# ---- the errors the GPU test is written for, made on oracle data (tests/test_headsets_host.py) ----
def _split(table, heads):
    out, c0 = {}, 0
    for h, c in heads.items():
        out[h] = table[:, c0:c0 + c]
        c0 += c
    return out


def _corrupt_group(ref, heads, group, kind):
    t = torch.from_numpy(channel_table(ref, heads, group))
    names, widths = list(heads), list(heads.values())
    starts = np.concatenate([[0], np.cumsum(widths)]).tolist()
    if kind == "swap_channels":  # two channels of the first head that has two
        j = next(i for i, c in enumerate(widths) if c >= 2)
        a = starts[j]
        t[:, [a, a + 1]] = t[:, [a + 1, a]]
    elif kind == "shift_after_first":  # an offset one too large for every head after the first
        c0 = widths[0]
        t[:, c0:] = torch.roll(t[:, c0:], -1, dims=1)
    elif kind == "zero_channel_3":  # the fourth output of the first 4-channel head never written
        j = widths.index(4)
        t[:, starts[j] + 3] = 0
    elif kind == "swap_heads":  # the first two heads of equal width trade places
        j, k = next((j, k) for j in range(len(names)) for k in range(j + 1, len(names)) if widths[j] == widths[k])
        a, b, c = starts[j], starts[k], widths[j]
        t[:, list(range(a, a + c)) + list(range(b, b + c))] = t[:, list(range(b, b + c)) + list(range(a, a + c))]
    else:
        raise KeyError(kind)
    return {f"{group}/{h}": v for h, v in _split(t, heads).items()}


CORRUPTIONS = ("swap_channels", "shift_after_first", "zero_channel_3", "swap_heads")


def applies(kind, heads):
    w = list(heads.values())
    return {"swap_channels": max(w) >= 2, "shift_after_first": len(w) >= 2, "zero_channel_3": 4 in w,
            "swap_heads": len(set(w)) < len(w)}[kind]


def corrupt(ref, heads, kind):
    """A copy of the oracle stage outputs `ref` with one error of `kind` in every group, as f32 (what a GPU
    forward would hand back)."""
    out = {}
    for g in GROUPS:
        out.update(_corrupt_group(ref, heads, g, kind))
    return {k: v.to(torch.float32) for k, v in out.items()}
