"""The validation tier on the host (no GPU): the numpy restatement (tests/loss_restatement.py) reproduces the
reference fixture (tests/golden/gen_loss_golden.py) — targets bit for bit, losses within the reference's own
float32 error — and the new entry points validate their arguments before any device call."""
import ctypes

import numpy as np
import pytest

import golden_io
import loss_restatement as lr
from conftest import GOLDEN
from sfa_hip import _lib

C, M = 3, 8
HEADS = ("hm_cen", "cen_offset", "direction", "z_coor", "dim")


@pytest.fixture(scope="module")
def g():
    return golden_io.load(GOLDEN, "loss_golden")


def case_names():
    return [str(n) for n in golden_io.load(GOLDEN, "loss_golden")["cases"]]


CASES = case_names()


def case_targets(g, name):
    return {k: g[f"{name}/t/{k}"] for k in lr.KEYS}


def case_loss_inputs(g, name):
    """(preds with the reference's clamped probabilities, targets as the loss part of the case uses them)."""
    preds = {h: g[f"{name}/logits/{h}"] for h in HEADS}
    preds["hm_cen"], preds["cen_offset"] = g[f"{name}/probs/hm_cen"], g[f"{name}/probs/cen_offset"]
    tg = case_targets(g, name)
    tg["obj_mask"], tg["indices_center"] = g[f"{name}/loss_mask"], g[f"{name}/loss_ind"]
    return preds, tg


def restated_targets(g, name):
    return lr.build_targets_batch(g[f"{name}/labels"], g[f"{name}/offsets"], g[f"{name}/flips"],
                                  hm_size=tuple(g[f"{name}/hm_size"]), num_classes=C, max_objects=M)


def test_fixture_covers_the_cases(g):
    assert str(g["numpy_version"]) == np.__version__, "the dtype chain follows numpy's promotion rules"
    hm = {n: g[f"{n}/t/hm_cen"] for n in CASES}
    ign = np.float32(0.9999)
    assert (hm["misc2432"] == ign).any() and (hm["order16"] == ign).any()
    # the same cell: 0.9999 where the ignore label came last, 1.0 where the real one did
    cell = np.unravel_index(np.argmax(hm["order16"][1, 1]), (16, 16))
    assert hm["order16"][1, 1][cell] == 1 and hm["order16"][2, 1][cell] == ign
    assert g["many16/labels"].shape[0] > M and g["many16/t/obj_mask"].sum() == M
    assert g["empty16/t/obj_mask"].sum() == 0 and not (hm["empty16"] == 1).any()
    assert not (hm["ignoreonly16"] == 1).any() and (hm["ignoreonly16"] == ign).any()
    assert g["misc2432/flips"].tolist() == [0, 1, 0] and g["misc2432/offsets"][-1] == g["misc2432/offsets"][-2]
    assert (g["outmap2432/t/indices_center"] >= 24 * 32).any() and g["outmap2432/status"].tolist() == [1, 1]
    assert {tuple(g[f"{n}/hm_size"]) for n in CASES} == {(16, 16), (24, 32)}


@pytest.mark.parametrize("name", CASES)
def test_restated_targets_equal_the_reference(g, name):
    got, status = restated_targets(g, name)
    np.testing.assert_array_equal(status, g[f"{name}/status"])
    for k in lr.KEYS:
        ref = g[f"{name}/t/{k}"]
        assert got[k].dtype == ref.dtype and got[k].shape == ref.shape, k
        if ref.dtype == np.float32:  # bit for bit: the restatement runs on the same numpy and libm
            np.testing.assert_array_equal(got[k].view(np.uint32), ref.view(np.uint32), err_msg=k)
        else:
            np.testing.assert_array_equal(got[k], ref, err_msg=k)


@pytest.mark.parametrize("name", CASES)
def test_restated_loss_within_the_reference_error(g, name):
    preds, tg = case_loss_inputs(g, name)
    mine, sums = lr.compute_loss(preds, tg)
    ref, d_ref = g[f"{name}/ref_loss"], g[f"{name}/d_ref"]
    assert np.all(np.abs(mine - ref) <= d_ref + 1e-6 * np.abs(ref)), (mine, ref)
    assert sums[2] == (tg["hm_cen"] == 1).sum() and sums[7] == tg["obj_mask"].sum()


def test_loss_cases_cover_the_branches(g):
    """num_pos == 0, an all-zero mask, |diff| on both sides of beta = 1, B = 1 and B = 3."""
    for name, want in (("empty16", True), ("ignoreonly16", True), ("borders16", False)):
        preds, tg = case_loss_inputs(g, name)
        _, sums = lr.compute_loss(preds, tg)
        assert (sums[2] == 0) == want and (sums[7] == 0) == want
    preds, tg = case_loss_inputs(g, "misc2432")
    diff = np.abs(lr._gather(preds["dim"].astype(np.float64), tg["indices_center"]) - tg["dim"])[tg["obj_mask"] == 1]
    assert (diff < 1).any() and (diff >= 1).any()
    assert {g[f"{n}/t/hm_cen"].shape[0] for n in CASES} >= {1, 3}


def _p(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def _params(**kw):
    p = _lib.SfaTargetParams()
    p.boundary = (ctypes.c_double * 6)(0, 50, -25, 25, -2.73, 1.27)
    p.hm_h, p.hm_w, p.num_classes, p.max_objects = 152, 152, 3, 50
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_build_targets_argument_errors():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = _p(buf)

    def call(prm, batch=2, labels=p, status=p):
        return L.sfa_build_targets(labels, p, 0, batch, ctypes.byref(prm) if prm is not None else None, p, p, p, p, p,
                                   p, p, status, None)

    for prm, kw in ((_params(hm_h=0), {}), (_params(hm_w=-1), {}), (_params(num_classes=0), {}),
                    (_params(num_classes=17), {}), (_params(max_objects=0), {}), (_params(max_objects=257), {}),
                    (_params(), {"batch": 0}), (_params(), {"batch": 65}), (_params(), {"labels": None}),
                    (_params(), {"status": None}), (None, {})):
        assert call(prm, **kw) == -1
        assert b"build_targets" in L.sfa_last_error_string()
    prm = _params()
    prm.reserved[3] = 1
    assert call(prm) == -1 and b"reserved" in L.sfa_last_error_string()
    assert call(_params(max_objects=300)) == -1 and b"max_objects" in L.sfa_last_error_string()


def test_compute_loss_argument_errors():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = _p(buf)
    need = L.sfa_compute_loss_workspace_size(2, 3, 152, 152, 50)
    assert need > 0

    def call(B=2, C=3, H=152, W=152, M=50, ws_bytes=need, first=p, ws=p):
        return L.sfa_compute_loss(first, p, p, p, p, p, p, p, p, p, p, p, B, C, H, W, M, 0, p, p, p, ws, ws_bytes, None)

    for kw in ({"B": 0}, {"B": 65}, {"C": 0}, {"C": 17}, {"H": 0}, {"W": -3}, {"M": 0}, {"M": 257}, {"first": None},
               {"ws": None}):
        assert call(**kw) == -1, kw
        assert b"compute_loss" in L.sfa_last_error_string()
    assert call(ws_bytes=need - 1) == -4 and b"workspace" in L.sfa_last_error_string()
    for bad in ((0, 3, 152, 152, 50), (65, 3, 152, 152, 50), (2, 17, 152, 152, 50), (2, 3, 152, 152, 257)):
        assert L.sfa_compute_loss_workspace_size(*bad) == 0


def test_workspace_size_is_monotone():
    L = _lib.lib()
    base = [2, 3, 96, 96, 50]
    steps = ([1, 2, 16, 64], [1, 3, 16], [1, 24, 152, 512], [1, 32, 152, 512], [1, 8, 50, 256])
    for axis, values in enumerate(steps):
        sizes = []
        for v in values:
            a = list(base)
            a[axis] = v
            sizes.append(L.sfa_compute_loss_workspace_size(*a))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, sizes)
    assert L.sfa_compute_loss_workspace_size(64, 16, 512, 512, 256) > L.sfa_compute_loss_workspace_size(1, 1, 1, 1, 1)


def test_abi_version_unchanged():
    assert _lib.lib().sfa_abi_version() == 2 == _lib.ABI_VERSION
    for s in ("sfa_build_targets", "sfa_compute_loss", "sfa_compute_loss_workspace_size"):
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), s)


def test_losses_module_refuses_cpu_and_grad():
    import torch
    from losses.losses import Compute_Loss, FocalLoss, L1Loss, L1Loss_Balanced, _neg_loss  # noqa: F401
    crit = Compute_Loss("cpu")
    outs = {h: torch.zeros(1, c, 4, 4) for h, c in zip(HEADS, (3, 2, 2, 1, 3))}
    tg = {"hm_cen": torch.zeros(1, 3, 4, 4)}
    with pytest.raises(_lib.SfaNativeError, match="GPU"):
        crit(outs, tg)
    outs["hm_cen"].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="evaluation only"):
        crit(outs, tg)
