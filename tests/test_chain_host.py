"""The chain restatement (tests/chain_restatement.py) on the CPU: pinned to the reference's recorded float32 run
(tests/golden/gen_chain_golden.py), the premises of the two cases, the gate condition, the eight wiring mutants the
gate has to catch, and a finite difference of the float64 loss.  case_reference() is what tests/test_gpu_chain.py
compares the GPU against."""
import functools

import numpy as np
import pytest
import torch

import chain_restatement as cr
import golden_io
from conftest import GOLDEN

CASES = list(cr.CASES)
LAYERS = ("layer1", "layer2", "layer3", "layer4")


@functools.lru_cache(maxsize=None)
def fixture():
    return golden_io.load(GOLDEN, "chain_golden")


@functools.lru_cache(maxsize=None)
def model_state():
    return cr.draw_model()


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """The float64 restatement from the fixture's image, computed once per process: inputs, loss, maps, grads (the 126
    parameters, "x", "pooled"), inter (pooled, out_layer1..4, up_level2..4), details (what the premises read), gate."""
    g, sd = fixture(), model_state()
    inp = cr.draw_inputs(case, g[f"{case}/image"])
    inter, details = {}, {}
    loss, maps, grads = cr.forward_backward(sd, inp["image"], inp["targets"], inter=inter, details=details)
    return dict(inputs=inp, loss=loss, maps=maps, grads=grads, inter=inter, details=details, gate=cr.gates(g, case))


def _fails_by(got, ref, gate, names):
    """The largest m / gate over ``names`` and both forms."""
    return max(float(np.max(cr.metric(got[k], ref[k]) / gate[k])) for k in names)


@pytest.mark.parametrize("case", CASES)
def test_float32_restatement_reproduces_the_reference(case):
    g, sd, r = fixture(), model_state(), case_reference(case)
    inp = r["inputs"]
    inter = {}
    loss, maps, grads = cr.forward_backward(sd, inp["image"], inp["targets"], dtype=torch.float32, inter=inter)
    _, _, cut = cr.forward_backward(sd, [inter[n] for n in LAYERS], inp["targets"], dtype=torch.float32)
    grads.update({n: cut[n] for n in LAYERS})
    assert len(grads) == 132 and all(v.dtype == np.float32 for v in grads.values())
    u = 2.0 ** -23
    assert np.all(np.abs(loss - g[f"{case}/loss"]) <= (2 * g[f"{case}/loss_noise32"] + u) * np.abs(g[f"{case}/loss"]))
    for h in cr.HEADS:
        assert np.all(cr.metric(maps[h], g[f"{case}/map/{h}"]) <= 2 * g[f"{case}/noise32/map/{h}"] + u), h
    for k, v in grads.items():
        n32 = float(g[f"{case}/noise32/{k}"][0])
        norm, samples, proj = cr.summary(k, v)
        ref_norm = float(g[f"{case}/norm/{k}"])
        assert abs(float(norm) - ref_norm) <= (2 * n32 + u) * ref_norm, k
        _, once = np.unique(cr.sample_indices(k, v.size), return_index=True)  # every sampled element counted once
        d = (samples.astype(np.float64) - g[f"{case}/samples/{k}"])[once]
        assert np.linalg.norm(d) <= (2 * n32 + u) * ref_norm, k
        assert np.all(np.abs(proj - g[f"{case}/proj/{k}"]) / ref_norm <= 2 * n32 + u), k


@pytest.mark.parametrize("case", CASES)
def test_premises(case):
    g, sd, r = fixture(), model_state(), case_reference(case)
    c, d = cr.CASES[case], r["details"]
    assert r["inter"]["pooled"].shape == (c["B"], 64, c["H"] // 4, c["W"] // 4)
    assert r["inter"]["layer4"].shape == (c["B"], 512, c["H"] // 32, c["W"] // 32)
    assert np.all(d["objects"] >= 3)
    assert np.all(r["loss"] != 0) and np.all(np.isfinite(r["loss"]))
    assert 1e-4 < d["gathered_sigmoid"].min() and d["gathered_sigmoid"].max() < 1 - 1e-4
    hm = 1 / (1 + np.exp(-r["maps"]["hm_cen"][r["inputs"]["targets"]["hm_cen"] == 1]))
    assert hm.size and 1e-4 < hm.min() and hm.max() < 1 - 1e-4  # the positive cells of the focal term
    for k in ("cen_offset", "direction", "z_coor", "dim"):
        assert d[f"diff/{k}"].min() > 1e-3, k
    # the gradient at each of the five output maps: a second backward from the maps, by the restatement's own loss
    maps = {h: torch.from_numpy(v).requires_grad_() for h, v in r["maps"].items()}
    with torch.enable_grad():
        cr.loss_terms(maps, cr._targets(r["inputs"]["targets"], torch.float64))[0].backward()
    assert all(float(t.grad.norm()) > 0 for t in maps.values())
    names = cr.parameter_names(sd)
    norms = np.array([np.linalg.norm(r["grads"][k]) for k in names])
    assert len(names) == 126 and norms.min() > 1e-6 * norms.max()
    # no ReLU and no pooling choice within MARGIN of changing: the gradient is continuous over the forward's deviation
    assert cr.margins(sd, r["inputs"]["image"]) >= cr.MARGIN
    assert float(g[f"{case}/margin"]) >= cr.MARGIN


@pytest.mark.parametrize("case", CASES)
def test_every_gate_is_at_most_one_percent(case):
    gate = case_reference(case)["gate"]
    assert len(gate) == 132 + 5
    worst = max(gate, key=lambda k: gate[k].max())
    print(f"{case}: widest gate {gate[worst].max():.3e} at {worst}")
    assert all(np.all(v > 0) and np.all(v <= cr.GATE_LIMIT) for v in gate.values()), worst


@pytest.mark.parametrize("mutant", cr.MUTANTS_RERUN + cr.MUTANTS_POST)
@pytest.mark.parametrize("case", CASES)
def test_the_gate_catches_the_mutant(case, mutant):
    sd, r = model_state(), case_reference(case)
    names = cr.parameter_names(sd) + ["x", "pooled"]
    if mutant in cr.MUTANTS_POST:
        got = cr.mutate_grads(r["grads"], mutant)
    else:
        _, _, got = cr.forward_backward(sd, r["inputs"]["image"], r["inputs"]["targets"], mutant=mutant)
    q = _fails_by(got, r["grads"], r["gate"], names)
    print(f"{case}/{mutant}: {q:.3g} x gate")
    assert q >= 10.0


def _group_direction(sd, group, seed):
    rng = np.random.default_rng([seed, sorted(("stem", "blocks", "neck", "heads")).index(group)])
    return {k: rng.integers(0, 2, np.shape(sd[k])) * 2.0 - 1.0 for k in cr.parameter_names(sd) if cr.group_of(k) == group}


@pytest.mark.parametrize("group", ["stem", "blocks", "neck", "heads"])
def test_finite_difference(group):
    """(L(theta + e d) - L(theta - e d)) / 2 e against <grad, d> along a seeded +-1 direction d over the group's
    parameters, e = 2e-7: the activations move by about 1e-5, far inside the margin, so L is smooth on the segment;
    the central difference's truncation error is O(e^2) and its rounding error about 1e-16 L / e = 1e-8 of L."""
    case = "c1_32x160"
    sd, r = model_state(), case_reference(case)
    inp, e = r["inputs"], 2e-7
    d = _group_direction(sd, group, 77)
    sd64 = {k: np.asarray(v, np.float64) if k in d else v for k, v in sd.items()}
    side = []
    for sign in (1.0, -1.0):
        moved = dict(sd64, **{k: sd64[k] + sign * e * d[k] for k in d})
        side.append(cr.forward_backward(moved, inp["image"], inp["targets"])[0][0])
    fd = (side[0] - side[1]) / (2 * e)
    ad = sum(float((r["grads"][k] * d[k]).sum()) for k in d)
    print(f"{group}: finite difference {fd:.10g}, autograd {ad:.10g}, relative {abs(fd - ad) / abs(ad):.2e}")
    assert abs(fd - ad) <= 1e-6 * abs(ad)
