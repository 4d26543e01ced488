"""SFA_MATH_FP16 on the GPU: the one-product kernels against the error budget of the arithmetic
(profiles/fp16_error_budget.json, from the CPU emulation tests/fp16_emulation.py) and against the emulation
itself on identical inputs.

Tolerances: 2 x the budget entry of the case and head for whole forwards (the factor covers the kernels' f32
accumulation order and the rare operand-rounding flips it causes downstream, neither of which the f64
emulation has); 1e-5 * max(1, |ref|), the project's per-kernel gate, for the heads kernel on the GPU's own
inputs (products of fp16 operands are exact in f32: only the f32 summation order differs)."""
import json
import os

import numpy as np
import pytest
import torch

import fp16_emulation as emu
import golden_cases as gc
from oracle import model_oracle
from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_WEIGHT_SEED = 2  # bench.BENCH_WEIGHT_SEED; bench_golden.npz records it (asserted below)


class Cfg(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def budget():
    with open(os.path.join(REPO, "profiles", "fp16_error_budget.json")) as f:
        return json.load(f)["cases"]


def make_model(golden, device, heads=None):
    from models.model_utils import create_model
    model = create_model(Cfg(arch="fpn_resnet_18", heads=dict(heads or gc.HEADS), head_conv=64, imagenet_pretrained=False))
    if heads is None:
        sd = gc.state_dict_np(golden.model)
    else:
        sd = synthetic.synthetic_state_dict(_lib.state_layout(_lib.make_arch(dict(heads))), 5)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(device).eval(), sd


def _run(model, x):
    with torch.no_grad():
        out = model(x)
    torch.cuda.synchronize()
    return {h: v.cpu().numpy() for h, v in out.items()}


def _bits_equal(a, b):
    return all(np.array_equal(a[h].view(np.uint32), b[h].view(np.uint32)) for h in a)


@pytest.mark.parametrize("case", list(gc.MODEL_CASES))
def test_forward_small_cases(golden, gpu, budget, case):
    """Tiles spanning several frames (AmaxRows), partial M tiles, the layer4 split-K."""
    model, _ = make_model(golden, gpu)
    x = torch.from_numpy(gc.model_input(case)).to(gpu)
    model.set_math("fp16x3")
    x3 = _run(model, x)
    model.set_math("fp16")
    assert model._engine(gpu).math == _lib.MATH_FP16
    h1 = _run(model, x)
    assert not _bits_equal(h1, x3), "fp16 mode produced the fp16x3 bits: the mode did not run"
    for h in gc.HEADS:
        ref = golden.model[f"{case}/{h}"]
        e1, e3 = emu.rel_err(h1[h], ref), emu.rel_err(x3[h], ref)
        print(f"{case} {h}: fp16 err {e1:.3g} (budget {budget[case]['fp16'][h]:.3g}), fp16x3 err {e3:.3g}")
        assert e1 <= 2 * budget[case]["fp16"][h], (h, e1)
        assert e1 > e3, (h, e1, e3)


@pytest.mark.parametrize("case", list(gc.MODEL_CASES))
def test_heads_kernel_on_identical_inputs(golden, gpu, case):
    """The fused heads kernel at one product against the emulation of conv3x3 -> bias -> ReLU -> 1x1 from the
    GPU's own up_level2/3/4 maps (frame scales from each map): the per-kernel gate."""
    model, sd = make_model(golden, gpu)
    model.set_math("fp16")
    model.capture_visualization = True
    _run(model, torch.from_numpy(gc.model_input(case)).to(gpu))
    viz = model.get_visualization_data()
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    for level in range(3):
        inp = viz["kfpn_features"][level].cpu().to(torch.float64)
        want = emu.head_level(sdt, inp, level, gc.HEADS, 1)
        for h in gc.HEADS:
            got = viz["fpn_outputs"][h][level].cpu().numpy()
            if level == 0:
                got = got[:, :, ::2, ::2]  # the capture repeats level 0 up to H/4 x W/4
            e = emu.rel_err(got, want[h].numpy())
            print(f"{case} level {level} {h}: heads kernel vs emulation {e:.3g}")
            assert e <= 1e-5, (level, h, e)


def test_splitk_ticket_and_reduce_forms_agree(golden, gpu):
    case = "b2_96"
    x = torch.from_numpy(gc.model_input(case)).to(gpu)
    outs = []
    for tickets in (0, 1):
        model, _ = make_model(golden, gpu)
        model.set_math("fp16")
        model._engine(gpu).set_option(_lib.OPT_SPLITK_TICKETS, tickets)
        outs.append(_run(model, x))
    assert _bits_equal(outs[0], outs[1])


def test_batch_invariance_and_determinism(golden, gpu):
    model, _ = make_model(golden, gpu)
    model.set_math("fp16")
    x = torch.from_numpy(gc.model_input("b2_96")).to(gpu)
    a, b = _run(model, x), _run(model, x)
    assert _bits_equal(a, b), "two runs differ"
    one = _run(model, x[:1].contiguous())
    assert _bits_equal(one, {h: v[:1] for h, v in a.items()}), "frame 0 alone differs from frame 0 of the batch"


def _match(got, ref):
    """(matched, {column group: max |d|}) over reference detections found with the same class at the same pixel."""
    cols = {"score": [0], "xy": [1, 2], "z": [3], "dim": [4, 5, 6], "dir": [7, 8]}
    matched, worst = 0, {k: 0.0 for k in cols}
    for f in range(ref.shape[0]):
        key = {(int(r[9]), int(np.floor(r[1])), int(np.floor(r[2]))): r for r in got[f]}
        for r in ref[f]:
            q = key.get((int(r[9]), int(np.floor(r[1])), int(np.floor(r[2]))))
            if q is None:
                continue
            matched += 1
            for k, c in cols.items():
                worst[k] = max(worst[k], float(np.max(np.abs(q[c].astype(np.float64) - r[c]))))
    return matched, worst


def test_big_m_kernels_bench_batch(gpu, golden_bench, budget):
    """R3_BODY and the tile_rows >= 50000 strip variants are selected from ~9 frames at 608 x 608: bench's 16
    frames with bench's weights, against the reference fixture."""
    g, bb = golden_bench, budget["bench"]
    assert int(g["weight_seed"]) == BENCH_WEIGHT_SEED
    assert bb["matched"] >= 400, "the emulation itself matches too few detections for an assertion"
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), seed=BENCH_WEIGHT_SEED)
    eng = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu, math=_lib.MATH_FP16)
    x = torch.from_numpy(synthetic.synthetic_bev(16, seed=1)).to(gpu)
    out = eng.forward(x)
    ys, xs = g["sample_yx"]
    for h in runtime.DEFAULT_HEADS:
        e = emu.rel_err(out[h].cpu().numpy()[:, :, ys, xs], g[f"bench/{h}/samples"])
        print(f"bench batch {h}: fp16 err at the sample points {e:.3g} (budget {bb['fp16'][h]:.3g})")
        assert e <= 2 * bb["fp16"][h], (h, e)
    hm = runtime.sigmoid_clamp_(out["hm_cen"].clone())
    off = runtime.sigmoid_clamp_(out["cen_offset"].clone())
    dets = runtime.decode(hm, off, out["direction"], out["z_coor"], out["dim"], K=50).cpu().numpy()
    matched, worst = _match(dets, g["bench/dets"])
    print(f"bench batch: {matched} of {bb['of']} reference detections matched (emulation {bb['matched']}); "
          f"max column deltas {worst} (budget {bb['columns']})")
    for k, v in worst.items():
        assert v <= 2 * bb["columns"][k], (k, v)
    assert matched >= 0.9 * bb["matched"], matched


def test_public_set_math(golden, gpu):
    x = torch.from_numpy(gc.model_input("b2_96")).to(gpu)
    m_eng, _ = make_model(golden, gpu)
    m_eng._engine(gpu).set_math(_lib.MATH_FP16)
    want = _run(m_eng, x)
    m_before, _ = make_model(golden, gpu)
    m_before.set_math("fp16")  # no engine yet: applies to the one the first forward creates
    assert _bits_equal(_run(m_before, x), want)
    m_after, _ = make_model(golden, gpu)
    x3 = _run(m_after, x)
    m_after.set_math("fp16")  # the existing engine
    assert _bits_equal(_run(m_after, x), want) and not _bits_equal(x3, want)
    m_after.set_math(_lib.MATH_FP16X3)
    assert _bits_equal(_run(m_after, x), x3)
    with pytest.raises(ValueError):
        m_after.set_math("fp17")


def test_graph_replay_equals_eager(golden, gpu):
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    packed = runtime.pack_state_dict(gc.state_dict_np(golden.model), arch)
    eng = runtime.KfpnEngine(arch, packed, gpu, math=_lib.MATH_FP16)
    p = runtime.DetectorPipeline(eng, 2, 96, 96, K=20)
    p.x.copy_(torch.from_numpy(gc.model_input("b2_96")))

    def fwd():
        p.engine.forward_into(p.x, p.outs, _lib.IN_NCHW3, p.ws, _lib.stream_ptr(p.dev))

    fwd()
    torch.cuda.synchronize()
    eager = {h: v.clone() for h, v in p.outs.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fwd()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd()
    for v in p.outs.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p.outs[h], eager[h]) for h in eager)


def test_three_heads_fall_back(golden, gpu):
    """Head counts other than 5 have no one-product heads kernel: the mode still runs (heads on fp16x3). No
    reference fixture for 3 heads: the GPU stays within 2 x the emulation's own error against an f64 forward
    of the same weights."""
    heads = {"hm_cen": 3, "cen_offset": 2, "z_coor": 1}
    model, sd = make_model(golden, gpu, heads)
    model.set_math("fp16")
    xn = gc.model_input("b2_96")
    got = _run(model, torch.from_numpy(xn).to(gpu))
    sdt = {k: torch.from_numpy(v) for k, v in sd.items()}
    want = emu.forward(sdt, torch.from_numpy(xn), heads, 1, head_terms=2)  # the documented fallback: heads fp16x3
    with torch.no_grad():
        ref = model_oracle.forward({k: (v.double() if v.is_floating_point() else v) for k, v in sdt.items()},
                                   torch.from_numpy(xn).double(), heads)
    for h in heads:
        own = emu.rel_err(want[h], ref[h].numpy())
        e = emu.rel_err(got[h], want[h])
        print(f"3 heads {h}: gpu vs emulation {e:.3g}, emulation vs f64 forward {own:.3g}")
        assert e <= 2 * own, (h, e, own)
