"""The loss gradient on the host (no GPU): the float64 closed form (tests/loss_grad_restatement.py) against the
reference's autograd gradients (tests/golden/gen_loss_grad_golden.py) and against a finite difference of the
forward restatement; the new entry points' argument checks; the default Compute_Loss still refuses grad.

Cases of the fixture (C = 3): generic (B 2, 8 x 8, M 4, restated targets, one frame flipped); noobj (num_pos == 0,
all masks 0, denominators 1e-4); dup (three set slots of one frame on one cell, a masked slot with index 0 and
garbage targets); saturated (logits of +-12 in hm_cen and cen_offset: gradient exactly 0 there); balanced (|d| on
both sides of 1 and exactly 0); nonsquare (B 1, 16 x 12, M 50); gtvalues (gt of 1, of 0.9999 and gaussian tails).
"""
import ctypes

import numpy as np
import pytest

import golden_io
import loss_grad_restatement as gr
import loss_restatement as lr
from conftest import GOLDEN
from sfa_hip import _lib

HEADS = gr.HEADS
SIG = ("hm_cen", "cen_offset")
CASES = ("generic", "noobj", "dup", "saturated", "balanced", "nonsquare", "gtvalues")


@pytest.fixture(scope="module")
def g():
    return golden_io.load(GOLDEN, "loss_grad_golden")


def case_inputs(g, name):
    """(logits, targets, s before the clamp, reference gradients) of one case."""
    logits = {h: g[f"{name}/logits/{h}"] for h in HEADS}
    tg = {k: g[f"{name}/t/{k}"] for k in lr.KEYS}
    s = {h: g[f"{name}/s/{h}"] for h in SIG}
    ref = {h: g[f"{name}/grad/{h}"] for h in HEADS}
    return logits, tg, s, ref


def probabilities(logits, s):
    """The operands of apply_sigmoid = 0: the clamped float32 probabilities in the two sigmoid heads."""
    preds = dict(logits)
    for h in SIG:
        preds[h] = np.clip(s[h], gr.LO, gr.HI)
    return preds


def test_fixture_covers_the_cases(g):
    assert [str(n) for n in g["cases"]] == list(CASES)
    assert str(g["numpy_version"]) == np.__version__
    shapes = {n: g[f"{n}/logits/hm_cen"].shape for n in CASES}
    assert shapes["generic"] == (2, 3, 8, 8) and shapes["nonsquare"] == (1, 3, 16, 12)
    assert g["generic/t/indices_center"].shape == (2, 4) and g["nonsquare/t/indices_center"].shape == (1, 50)
    assert g["noobj/t/obj_mask"].sum() == 0 and not (g["noobj/t/hm_cen"] == 1).any()
    ind, mask = g["dup/t/indices_center"][0], g["dup/t/obj_mask"][0]
    assert ind.tolist() == [27, 27, 27, 0] and mask.tolist() == [1, 1, 1, 0] and g["dup/t/dim"][0, 3, 0] == 1e6
    for h in SIG:
        s = g[f"saturated/s/{h}"]
        assert (s > gr.HI).any() and (s < gr.LO).any() and ((s > gr.LO) & (s < gr.HI)).any()
        assert np.abs(g[f"saturated/logits/{h}"]).max() == 12
    for n in CASES:
        if n != "saturated":
            assert all(np.abs(g[f"{n}/logits/{h}"]).max() <= 8 for h in SIG)
    logits, tg, _, _ = case_inputs(g, "balanced")
    d = np.abs(lr._gather(logits["dim"].astype(np.float64), tg["indices_center"]) - tg["dim"])[tg["obj_mask"] == 1]
    assert (d == 0).any() and ((d > 0) & (d < 1)).any() and (d > 1).any()
    gt = g["gtvalues/t/hm_cen"]
    assert (gt == 1).any() and (gt == np.float32(0.9999)).any() and ((gt > 0) & (gt < 0.01)).any()
    assert len(np.unique(gt)) > 8
    # one regression cell of nonsquare is shared by two slots
    live = g["nonsquare/t/indices_center"][0][g["nonsquare/t/obj_mask"][0] == 1]
    assert len(set(live.tolist())) < len(live)


def test_no_fixture_sigmoid_is_within_two_ulp_of_a_clamp_edge(g):
    """The GPU bound lets s move by 2 ulp; an s that close to an edge could switch its gradient on or off."""
    for n in CASES:
        for h in SIG:
            s = g[f"{n}/s/{h}"]
            for edge in (gr.LO, gr.HI):
                lo, hi = gr.ulp_shift(edge, -3), gr.ulp_shift(edge, 3)
                assert not ((s >= lo) & (s <= hi)).any(), (n, h)


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_gradients(g, name):
    """The project's per-kernel gate, <= 1e-5 max(1, |ref|) per element, with the fixture's own s."""
    logits, tg, s, ref = case_inputs(g, name)
    mine = gr.compute_loss_grad(logits, tg, True, s)
    for h in HEADS:
        err = np.abs(mine[h] - ref[h]) / np.maximum(1.0, np.abs(ref[h]))
        print(f"loss_grad[{name}/{h}]: max gated error {err.max():.3e}, max |ref| {np.abs(ref[h]).max():.3e}")
        assert mine[h].shape == ref[h].shape and err.max() <= 1e-5, (name, h, err.max())
    if name == "saturated":
        for h in SIG:
            out = (s[h] < gr.LO) | (s[h] > gr.HI)
            assert np.all(mine[h][out] == 0) and np.all(ref[h][out] == 0)
    if name == "noobj":
        assert all(np.all(mine[h] == 0) for h in HEADS[1:])


def test_duplicates_add_up_and_masked_slots_do_not(g):
    logits, tg, s, _ = case_inputs(g, "dup")
    mine = gr.compute_loss_grad(probabilities(logits, s), tg)
    total = np.zeros(3)
    for k in range(3):  # each of the three slots alone, rescaled to the full mask sum's denominator
        one = dict(tg, obj_mask=np.zeros_like(tg["obj_mask"]))
        one["obj_mask"][0, k] = 1
        part = gr.compute_loss_grad(probabilities(logits, s), one)["dim"][0].reshape(3, -1)[:, 27]
        total += part * (1 * 3 + 1e-4) / (tg["obj_mask"].sum() * 3 + 1e-4)
    np.testing.assert_allclose(mine["dim"][0].reshape(3, -1)[:, 27], total, rtol=1e-14)
    assert np.all(mine["dim"][0].reshape(3, -1)[:, 0] == 0)  # the masked slot's cell


def test_gradient_equals_a_finite_difference_of_the_forward(g):
    """apply_sigmoid = 0 on the generic case: central differences of loss_restatement.compute_loss in float64.
    With e the float64 epsilon the step is h = e^(1/3) * scale (scale = min(p, 1 - p) for a probability, whose
    terms are singular at 0 and 1; 1 elsewhere).  Bound per element: truncation h^2 |f'''| / 6, which is at most
    10 e^(2/3) |g| for the focal terms (derivatives of log p, 1 / p fall like scale^-n), 0 for the piecewise
    linear L1 and at most (alpha b^3 / 3) e^(2/3) / den for balanced L1 (|f'''| <= 2 alpha b^3); plus the
    rounding of the two forward sums, 8 e sum|loss terms| / h."""
    logits, tg, s, _ = case_inputs(g, "generic")
    preds = {h: v.astype(np.float64) for h, v in probabilities(logits, s).items()}
    mine = gr.compute_loss_grad(preds, tg)
    e = np.finfo(np.float64).eps
    delta = e ** (1 / 3)
    base, _ = lr.compute_loss(preds, tg)
    lsum = float(np.abs(base[1:]).sum())
    msum = float(tg["obj_mask"].sum())
    checked = 0
    for h in HEADS:
        flat = preds[h].reshape(-1)
        got = mine[h].reshape(-1)
        c = preds[h].shape[1]
        for i in range(flat.size):
            x = flat[i]
            scale = min(x, 1 - x) if h in SIG else 1.0
            step = delta * scale
            flat[i] = x + step
            up = lr.compute_loss(preds, tg)[0][0]
            flat[i] = x - step
            dn = lr.compute_loss(preds, tg)[0][0]
            flat[i] = x
            fd = (up - dn) / ((x + step) - (x - step))
            bound = 10 * delta ** 2 * abs(got[i]) + 8 * e * lsum / step
            if h in ("z_coor", "dim"):
                bound += gr.ALPHA * gr.BB ** 3 / 3 * delta ** 2 / (msum * c + 1e-4)
            assert abs(fd - got[i]) <= bound, (h, i, fd, got[i], bound)
            checked += abs(got[i]) > 100 * bound
    assert checked > 200  # the check is not vacuous: most nonzero elements are far above their bound


def _p(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def test_grad_workspace_size_is_monotone_and_zero_out_of_range():
    L = _lib.lib()
    base = [2, 3, 96, 96, 50]
    steps = ([1, 2, 16, 64], [1, 3, 16], [1, 24, 152, 512], [1, 32, 152, 512], [1, 8, 50, 256])
    for axis, values in enumerate(steps):
        sizes = []
        for v in values:
            a = list(base)
            a[axis] = v
            sizes.append(L.sfa_compute_loss_grad_workspace_size(*a))
        assert all(sz > 0 and sz % 8 == 0 for sz in sizes) and sizes == sorted(sizes), (axis, sizes)
    assert (L.sfa_compute_loss_grad_workspace_size(64, 16, 512, 512, 256)
            > L.sfa_compute_loss_grad_workspace_size(1, 1, 1, 1, 1))
    for bad in ((0, 3, 152, 152, 50), (65, 3, 152, 152, 50), (2, 17, 152, 152, 50), (2, 3, 152, 152, 257),
                (2, 3, 8192, 8192, 50), (2, 3, 0, 152, 50), (2, 3, 152, 152, 0)):
        assert L.sfa_compute_loss_grad_workspace_size(*bad) == 0


def test_grad_argument_errors_before_any_launch():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = _p(buf)
    need = L.sfa_compute_loss_grad_workspace_size(2, 3, 152, 152, 50)

    def call(B=2, C=3, H=152, W=152, M=50, ws_bytes=need, first=p, ws=p, g_dim=p, status=p):
        return L.sfa_compute_loss_grad(first, p, p, p, p, p, p, p, p, p, p, p, B, C, H, W, M, 1, p, p, p, p, g_dim,
                                       status, ws, ws_bytes, None)

    for kw in ({"B": 0}, {"B": 65}, {"C": 0}, {"C": 17}, {"H": 0}, {"W": -3}, {"M": 0}, {"M": 257}, {"first": None},
               {"ws": None}, {"g_dim": None}, {"status": None}):
        assert call(**kw) == -1, kw
        assert b"compute_loss_grad" in L.sfa_last_error_string()
    assert call(ws_bytes=need - 1) == -4 and b"workspace" in L.sfa_last_error_string()


def test_abi_version_unchanged_and_symbols_present():
    import os
    import re
    from conftest import REPO
    assert _lib.lib().sfa_abi_version() == 2 == _lib.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sfa_hip.h")).read(), flags=re.S)
    for sym in ("sfa_compute_loss_grad", "sfa_compute_loss_grad_workspace_size"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), sym)
        assert re.search(r"\b%s\s*\(" % sym, header)


def test_default_mode_still_refuses_grad_and_grad_mode_refuses_cpu():
    import torch
    from losses.losses import Compute_Loss
    outs = {h: torch.zeros(1, c, 4, 4) for h, c in zip(HEADS, (3, 2, 2, 1, 3))}
    tg = {"hm_cen": torch.zeros(1, 3, 4, 4)}
    outs["hm_cen"].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="evaluation only"):
        Compute_Loss("cpu")(outs, tg)
    with pytest.raises(_lib.SfaNativeError, match="GPU"):  # no CPU fallback in the differentiable mode either
        Compute_Loss("cpu", differentiable=True)(outs, tg)
