"""Every rule of the body-conv table (csrc/conv_plan.h body_conv_rule, csrc/conv.hip launch_conv_h) on the GPU at the
smallest maps that reach it (tests/conv_dispatch_cases.py; tests/test_conv_dispatch_host.py proves on the CPU that the
table leaves no reachable rule out), and the whole model at the three input sizes where layer3 / layer4 change rule.

Block operator: engine.block_forward against the float64 restatement (tests/block_restatement.py conv3 on the folded
float32 parameters): mid judged from x, y from the device's own mid, at the stage gate 1e-5 max(1, |ref|) per element,
as test_gpu_block.test_forward_at_the_stage_gate does.  B = 2 with frame 1 scaled by 2^-6, so a 128-row tile straddles
two frames of different fp16x3 scales (3125 and 3124 rows are no multiple of 128); outputs in NaN-filled buffers
between guard bands; each frame bit-equal to the same frame run alone.

Whole model: gpu_maps / check_stages of tests/test_gpu_model_stages.py (f64 oracle stages on the GPU's own stage
inputs).  Mixed batches are judged per frame, single natural-amplitude frames per element, as that file does.
"""
import numpy as np
import pytest
import torch

import block_restatement as br
import conv_dispatch_cases as cd
import stage_cases as sc
import test_gpu_block as tb
import test_gpu_model_stages as ms
from test_gpu_model_stages import engine, sd64  # noqa: F401  (module-scoped fixtures)
from sfa_hip import _lib

pytestmark = pytest.mark.gpu

GATE = sc.GATE
_CACHE = {}


def block_input(layer, block, h, w):
    """Standard-normal NHWC frames, frame b times stage_cases.FACTORS[b] (1, 2^-6)."""
    cin = br.block_shape(layer, block)[0]
    rng = np.random.default_rng(7000 + 100 * layer + 10 * block + h)
    x = rng.standard_normal((cd.BATCH, h, w, cin)).astype(np.float32)
    return x * np.float32(sc.FACTORS[:cd.BATCH])[:, None, None, None]


def _run(gpu, layer, block, x):
    """block_forward into NaN-filled guarded buffers -> (mid, y) as numpy; every element written, no guard touched."""
    eng = tb._engine(gpu)
    _, cout, s, _ = br.block_shape(layer, block)
    B, h, w, _ = x.shape
    osh = (B, -(-h // s), -(-w // s), cout)
    g = tb.Guarded(gpu, [osh, osh], [True, True])
    eng.block_forward(layer, block, tb._dev(gpu, x), out=(g.outs[0], g.outs[1]))
    torch.cuda.synchronize()
    assert g.intact(), "a guard band was written"
    mid, y = g.outs[0].cpu().numpy(), g.outs[1].cpu().numpy()
    assert np.isfinite(mid).all() and np.isfinite(y).all(), "an element was not written"
    return mid, y


def _over_gate(got, ref):
    return float(np.max(np.abs(got - ref) / (GATE * np.maximum(1.0, np.abs(ref)))))


@pytest.mark.parametrize("case", range(len(cd.BLOCK_CASES)), ids=[f"layer{L}.{b}-{h}x{w}" for (L, b, (h, w)), _ in cd.BLOCK_CASES])
def test_block_rule_at_the_stage_gate(gpu, case):
    (layer, block, (h, w)), rules = cd.BLOCK_CASES[case]
    _, _, s, _ = br.block_shape(layer, block)
    f = br.fold(tb._params(layer, block))
    x = block_input(layer, block, h, w)
    mid, y = _run(gpu, layer, block, x)
    # the premise, from the device's maps: the two frames of both convs' inputs have different binary exponents
    for name, t in (("x", x), ("mid", mid)):
        e = sc.frame_exponents(t)
        assert e[0] is not None and e[1] is not None and e[0] != e[1], (name, e)
    x64 = x.astype(np.float64)
    rmid = np.maximum(br.conv3(x64, f["W1"], s) + f["b1"].astype(np.float64), 0.0)
    skip = x64 if f["Wd"] is None else x64[:, ::s, ::s] @ f["Wd"].astype(np.float64).T
    ry = np.maximum(br.conv3(mid, f["W2"], 1) + f["b2"].astype(np.float64) + skip, 0.0)
    q = (_over_gate(mid, rmid), _over_gate(y, ry))
    print(f"conv dispatch layer{layer}.{block} {cd.BATCH} x {h} x {w} ({rules[0]}, {rules[1]}): error / gate mid {q[0]:.3f} y {q[1]:.3f}")
    assert max(q) <= 1.0, q
    for b in range(cd.BATCH):
        m1, y1 = _run(gpu, layer, block, x[b:b + 1])
        assert np.array_equal(m1[0], mid[b]) and np.array_equal(y1[0], y[b]), f"frame {b} in the batch differs from the frame alone"


# ---------------------------------------------------------------- the whole model

def _input(H, W):
    if (H, W) not in _CACHE:
        _CACHE[(H, W)] = sc.mixed_batch(2, H, W, 71)  # frames scaled 1 and 2^-6
    return _CACHE[(H, W)]


def _with_option(eng, key, value, x):
    old = eng.get_option(key)
    eng.set_option(key, value)
    try:
        return ms.gpu_maps(eng, x)
    finally:
        eng.set_option(key, old)


def test_model_800_mixed_batch_every_stage(engine, sd64):  # noqa: F811
    """2 x 800 x 800 (the Argoverse configuration), production options: OW = 200 and 100 put the level-2 skip conv on
    fpn_gemm<64,64,true,3> and the level-1 one on fpn_row; every stage against the f64 oracle."""
    maps = ms.gpu_maps(engine, _input(800, 800))
    ms.assert_premise(maps, "800")
    ms.check_stages(maps, sd64, "fp16x3 mixed_2x800x800", True)


def test_model_896_layer3_on_the_large_map_rules(engine, sd64):  # noqa: F811
    """1 x 896 x 896: layer3's map has 3136 pixels, so its strip convs take <128,128> with C = 256 and layer3.0 takes
    R3_BODY with N = 256.  layer2..4 at the gate; the model with W images (layer3's image is 128 wide, so the <128,128>
    image instance reads it, on 256 channels for the first time) bit-equal to the model without images; a frame of a
    mixed batch of 2 bit-equal to itself alone."""
    x = _input(896, 896)
    full = ms.gpu_maps(engine, x)
    ms.assert_premise(full, "896")
    alone = [ms.gpu_maps(engine, x[b:b + 1]) for b in range(2)]
    ms.check_stages(alone[0], sd64, "fp16x3 1x896x896", False, only=("layer2", "layer3", "layer4"))
    for b in range(2):
        ms.assert_same_bits(full, alone[b], f"896 frame {b} in the batch vs alone", slice(b, b + 1))
    assert engine.get_option(_lib.OPT_W_IMAGES) == 1
    plain = _with_option(engine, _lib.OPT_W_IMAGES, 0, x[:1])
    ms.assert_same_bits(alone[0], plain, "896: W images 1 vs 0")


def test_model_1792_layer4_on_the_large_map_rules(engine, sd64):  # noqa: F811
    """1 x 1792 x 1792: layer4's map has 3136 pixels, so its strip convs take <128,128> with two K slices and layer4.0
    R3_BODY with two.  layer4 at the gate; split-K tickets 1 (the in-kernel combine) bit-equal to 0 (the reduce launch)
    on every map; a second forward in the same workspace bit-equal to the first (the tickets were zeroed again)."""
    x = torch.from_numpy(_input(1792, 1792)[:1]).to(engine.device)
    maps = ms.gpu_maps(engine, x)
    ms.check_stages(maps, sd64, "fp16x3 1x1792x1792", False, only=("layer4",))
    reduce = ms.gpu_maps(engine, x, opts=(1, 7, 61, 0))
    ms.assert_same_bits(maps, reduce, "1792: split-K tickets 1 vs 0")
    for k, v in zip(ms.OPTS, ms.PRODUCTION):
        engine.set_option(k, v)
    dev = engine.device
    with torch.cuda.device(dev):
        ws = torch.empty(engine.workspace_bytes(1, 1792, 1792), dtype=torch.uint8, device=dev)
        runs = []
        for _ in range(2):
            outs = engine.alloc_outputs(1, 1792, 1792)
            engine.forward_into(x, outs, workspace=ws)
            torch.cuda.synchronize()
            v = engine.debug_views(ws, 1, 1792, 1792)
            runs.append(dict({f"out/{h}": outs[h] for h in ms.HEADS}, layer4=v["layer4"].contiguous().clone()))
    ms.assert_same_bits(runs[0], runs[1], "1792: second forward in the same workspace")
    ms.assert_same_bits(runs[0], {k: maps[k] for k in runs[0]}, "1792: forward in a fresh workspace")
