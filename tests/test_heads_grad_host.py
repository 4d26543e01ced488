"""Head parameter gradients, CPU side: the numpy float64 restatement (tests/heads_grad_restatement.py) against the
reference's own autograd (tests/golden/heads_grad_golden.npz), against a central finite difference of its own
forward, its known answers, the symbols, and tools/heads_grad_plan_check.cpp under the host sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import golden_io
import heads_grad_restatement as hr
from conftest import GOLDEN, REPO

HEADS = ("hm_cen", "cen_offset", "direction", "z_coor", "dim")


@pytest.fixture(scope="module")
def fixture():
    return golden_io.load(GOLDEN, "heads_grad_golden")


def test_restatement_meets_the_gate_against_the_reference(fixture):
    misses = []
    cases = [str(c) for c in fixture["cases"]]
    assert {int(fixture[f"{c}/level"]) for c in cases} == {0, 1, 2} and "L1_5x7" in cases
    for c in cases:
        x = fixture[f"{c}/x"]
        assert x.shape[0] == 2 and x.shape[3] == (256, 128, 64)[int(fixture[f"{c}/level"])]
        for n in HEADS:
            W1, b1, W2, b2, g = (fixture[f"{c}/{n}/{k}"] for k in ("W1", "b1", "W2", "b2", "g"))
            A, Hd, y = hr.forward(x, W1, b1, W2, b2)
            assert np.abs(A).min() >= 1e-4  # the generator's condition: no ReLU edge in the case
            r = hr.grads(x, Hd, W2, g)
            for key, mine in (("y", y), ("dW1", r["dW1"]), ("db1", r["db1"]),
                              ("dW2", r["dW2"].reshape(fixture[f"{c}/{n}/dW2"].shape)), ("db2", r["db2"])):
                worst, ok = hr.gate(fixture[f"{c}/{n}/{key}"], mine)
                if not ok:
                    misses.append((c, n, key, worst))
    assert not misses, misses


def test_fixture_records_the_references_own_error(fixture):
    """d_ref, the reference's float32 distance from the float64 restatement when the fixture was generated (y, dW1,
    db1, dW2, db2, relative to max(1, |r|)), is what the restatement finds again, and lies inside the gate."""
    for c in (str(c) for c in fixture["cases"]):
        x, d_ref = fixture[f"{c}/x"], fixture[f"{c}/d_ref"]
        assert d_ref.shape == (5,) and np.all(d_ref > 0) and np.all(d_ref <= 1e-5)
        mine = np.zeros(5)
        for n in HEADS:
            W1, b1, W2, b2, g = (fixture[f"{c}/{n}/{k}"] for k in ("W1", "b1", "W2", "b2", "g"))
            _, Hd, y = hr.forward(x, W1, b1, W2, b2)
            r = hr.grads(x, Hd, W2, g)
            want = (y, r["dW1"], r["db1"], r["dW2"].reshape(fixture[f"{c}/{n}/dW2"].shape), r["db2"])
            for k, key in enumerate(("y", "dW1", "db1", "dW2", "db2")):
                mine[k] = max(mine[k], hr.gate(fixture[f"{c}/{n}/{key}"], want[k])[0])
        assert np.allclose(mine, d_ref, rtol=1e-6, atol=0), (c, mine, d_ref)


def test_restatement_equals_its_finite_difference():
    """d (sum y g) / d theta by a central difference in float64.  The forward is piecewise quadratic in each single
    parameter; away from a ReLU edge the central difference of a quadratic is exact, so the error is the rounding of
    the two evaluations: |F| ~ sum|y g| carries about n eps |F| with n the terms, divided by 2 step."""
    rng = np.random.default_rng(1)
    B, h, w, C, O, c = 2, 4, 5, 6, 8, 3
    x = rng.standard_normal((B, h, w, C))
    W1, b1 = rng.standard_normal((O, C, 3, 3)) * 0.3, rng.standard_normal(O)
    W2, b2 = rng.standard_normal((c, O)), rng.standard_normal(c)
    g = rng.standard_normal((B, c, h, w))
    A, Hd, y = hr.forward(x, W1, b1, W2, b2)
    step = 1e-6
    assert np.abs(A).min() > 50 * step * (1 + np.abs(x).max() * 1)  # no pre-activation changes sign inside a step
    r = hr.grads(x, Hd, W2, g, dA32=hr.dhidden(Hd, W2, g)[0])  # float64 throughout: dA not rounded
    F = lambda *p: float((hr.forward(x, *p)[2] * g).sum())  # noqa: E731
    scale = float(np.abs(y * g).sum()) + 1.0
    tol = 9 * C * O * 2.0 ** -52 * scale / step  # terms of one y element ~ 9 C O; two evaluations over 2 step
    params = [W1, b1, W2, b2]
    for k, key in enumerate(("dW1", "db1", "dW2", "db2")):
        flat = params[k].reshape(-1)
        for idx in rng.choice(flat.size, size=min(12, flat.size), replace=False):
            keep = flat[idx]
            flat[idx] = keep + step
            up = F(*params)
            flat[idx] = keep - step
            dn = F(*params)
            flat[idx] = keep
            fd = (up - dn) / (2 * step)
            assert abs(fd - r[key].reshape(-1)[idx]) <= tol, (key, idx, fd, r[key].reshape(-1)[idx], tol)


@pytest.mark.parametrize("pos", [(0, 0, 0), (1, 2, 3), (1, 4, 6)])
def test_one_hot_known_answer(pos):
    B, h, w, C, O = 2, 5, 7, 8, 4
    x, dA, want = hr.one_hot_case(B, h, w, C, O, *pos, o0=2)
    assert np.unique(x).size == x.size
    # W2 = identity column, g one-hot, Hd = 1: the restatement's own dA is the one-hot, and dW1 the shifted copy
    W2 = np.zeros((1, O))
    W2[0, 2] = 1.0
    g = np.zeros((B, 1, h, w))
    g[pos[0], 0, pos[1], pos[2]] = 1.0
    r = hr.grads(x, np.ones((B, h, w, O)), W2, g)
    assert np.array_equal(r["dA32"], dA) and np.array_equal(r["dW1"].astype(np.float32), want)
    assert np.array_equal(r["db1"], dA[pos]) and r["dW2"][0, 2] == 1.0 and r["db2"][0] == 1.0
    if pos == (0, 0, 0):  # the corner: the taps above and left of the map are zero
        assert not want[2, :, 0, :].any() and not want[2, :, :, 0].any() and want[2, :, 1, 1].any()


def test_symbols_declared_and_bound():
    from sfa_hip import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sfa_hip.h")).read(), flags=re.S)
    for sym in ("sfa_model_heads_grad", "sfa_model_heads_grad_workspace_size", "sfa_model_heads_grad_chunk_pixels"):
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), sym)
    from sfa_hip.runtime import KfpnEngine
    assert hasattr(KfpnEngine, "heads_param_grad")


def test_plan_check_under_host_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "heads_grad_plan_check")
    cmd = [gxx, "-std=c++17", "-g", "-O2", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "heads_grad_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0"))
    assert r.returncode == 0 and " plans, 0 bad" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
