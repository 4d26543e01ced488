"""The heads' input gradient, CPU side: the numpy float64 restatement (tests/heads_dgrad_restatement.py) against the
reference's own autograd x.grad (tests/golden/heads_dgrad_golden.npz), against a central finite difference of the
forward restatement, its one-hot known answers, and the new symbols and methods."""
import glob
import os
import re

import numpy as np
import pytest

import golden_io
import heads_dgrad_restatement as dr
import heads_grad_restatement as hr
from conftest import GOLDEN, REPO

HEADS = ("hm_cen", "cen_offset", "direction", "z_coor", "dim")


@pytest.fixture(scope="module")
def fixture():
    return golden_io.load(GOLDEN, "heads_dgrad_golden")


def _case(fixture, c):
    """(x, dA of all heads side by side (float64, not rounded), W1 of all heads, per-head y restated)."""
    x = fixture[f"{c}/x"]
    dA, W1s, ys = [], [], {}
    for n in HEADS:
        W1, b1, W2, b2, g = (fixture[f"{c}/{n}/{k}"] for k in ("W1", "b1", "W2", "b2", "g"))
        A, Hd, y = hr.forward(x, W1, b1, W2, b2)
        assert np.abs(A).min() >= 1e-4  # the generator's condition: no ReLU edge in the case
        y2, _ = dr.head_out(Hd, W2, b2)
        assert np.allclose(y2, y, rtol=1e-13, atol=1e-13)  # the two restatements of y agree
        dA.append(hr.dhidden(Hd, W2, g)[0])
        W1s.append(W1)
        ys[n] = y
    return x, np.concatenate(dA, axis=3), np.concatenate(W1s, axis=0), ys


def test_restatement_meets_the_gate_against_the_reference(fixture):
    cases = [str(c) for c in fixture["cases"]]
    assert {int(fixture[f"{c}/level"]) for c in cases} == {0, 1, 2} and "L1_5x7" in cases
    misses = []
    for c in cases:
        x, dA, W1, ys = _case(fixture, c)
        assert x.shape[0] == 2 and x.shape[3] == (256, 128, 64)[int(fixture[f"{c}/level"])]
        dX, _ = dr.dgrad(dA, W1)
        worst = [max(hr.gate(fixture[f"{c}/{n}/y"], ys[n])[0] for n in HEADS), hr.gate(fixture[f"{c}/dx"], dX)[0]]
        d_ref = fixture[f"{c}/d_ref"]
        assert d_ref.shape == (2,) and np.all(d_ref > 0) and np.allclose(worst, d_ref, rtol=1e-6, atol=0), (c, worst)
        for key, v in zip(("y", "dx"), worst):
            if not v <= 1e-5:
                misses.append((c, key, v))
    assert not misses, misses


def test_restatement_equals_its_finite_difference():
    """d (sum_heads sum y g) / d x by a central difference in float64: the forward is piecewise linear in a single
    input element, so away from a ReLU edge the central difference is exact up to the rounding of the two
    evaluations, about n eps |F| with n the terms of one y element, divided by 2 step."""
    rng = np.random.default_rng(2)
    B, h, w, C, O, c, nh = 2, 4, 5, 6, 8, 3, 2
    x = rng.standard_normal((B, h, w, C))
    heads = [(rng.standard_normal((O, C, 3, 3)) * 0.3, rng.standard_normal(O), rng.standard_normal((c, O)),
              rng.standard_normal(c), rng.standard_normal((B, c, h, w))) for _ in range(nh)]
    step = 1e-6
    dA, scale = [], 1.0
    for W1, b1, W2, b2, g in heads:
        A, Hd, y = hr.forward(x, W1, b1, W2, b2)
        assert np.abs(A).min() > 50 * step * np.abs(W1).max()  # no pre-activation changes sign inside a step
        dA.append(hr.dhidden(Hd, W2, g)[0])
        scale += float(np.abs(y * g).sum())
    dX, _ = dr.dgrad(np.concatenate(dA, axis=3), np.concatenate([hd[0] for hd in heads], axis=0))
    F = lambda xv: sum(float((hr.forward(xv, W1, b1, W2, b2)[2] * g).sum()) for W1, b1, W2, b2, g in heads)  # noqa: E731
    tol = 9 * C * O * 2.0 ** -52 * scale / step
    flat = x.reshape(-1)
    for idx in rng.choice(flat.size, size=24, replace=False):
        keep = flat[idx]
        flat[idx] = keep + step
        up = F(x)
        flat[idx] = keep - step
        dn = F(x)
        flat[idx] = keep
        fd = (up - dn) / (2 * step)
        assert abs(fd - dX.reshape(-1)[idx]) <= tol, (idx, fd, dX.reshape(-1)[idx], tol)


@pytest.mark.parametrize("pos", [(0, 0, 0), (1, 2, 3), (1, 4, 6)])
def test_one_hot_known_answer(pos):
    B, h, w, C, O = 2, 5, 7, 8, 4
    W1, dA, want = dr.one_hot_case(B, h, w, C, O, *pos, o0=2)
    assert np.unique(W1).size == W1.size
    dX, S = dr.dgrad(dA, W1)
    assert np.array_equal(dX.astype(np.float32), want) and np.array_equal(S, np.abs(dX))
    b0, y0, x0 = pos
    assert np.count_nonzero(want) == sum(C for ky in range(3) for kx in range(3)
                                         if 0 <= y0 + ky - 1 < h and 0 <= x0 + kx - 1 < w)
    assert np.array_equal(want[b0, y0, x0], W1[2, :, 1, 1])
    if pos == (0, 0, 0):  # the corner: the taps ky = 0 and kx = 0, which would land above or left of the map, are absent
        assert np.count_nonzero(want) == 4 * C
        assert np.array_equal(want[0, 1, 1], W1[2, :, 2, 2]) and np.array_equal(want[0, 0, 1], W1[2, :, 1, 2])
        assert np.array_equal(want[0, 1, 0], W1[2, :, 2, 1])
    if pos == (1, 2, 3):
        assert np.array_equal(want[1, 1, 2], W1[2, :, 0, 0]) and np.array_equal(want[1, 3, 4], W1[2, :, 2, 2])


def test_symbols_declared_and_bound():
    from sfa_hip import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sfa_hip.h")).read(), flags=re.S)
    for sym in ("sfa_model_heads_input_grad", "sfa_model_heads_forward", "sfa_model_heads_forward_workspace_size",
                "sfa_heads_dgrad_pixel_tile"):
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), sym)
    assert re.search(r"#define\s+SFA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    assert _lib.lib().sfa_abi_version() == 2
    (plan_h,) = glob.glob(os.path.join(REPO, "*", "csrc", "heads_grad_plan.h"))
    plan = open(plan_h).read()
    m = re.search(r"constexpr int kHgDgPix = (\d+);", plan)
    assert m and _lib.heads_dgrad_pixel_tile() == int(m.group(1))
    from sfa_hip.runtime import KfpnEngine
    from models.fpn_resnet import PoseResNet
    assert hasattr(KfpnEngine, "heads_input_grad") and hasattr(KfpnEngine, "heads_forward")
    assert hasattr(PoseResNet, "level_heads") and hasattr(PoseResNet, "heads_from_levels")
