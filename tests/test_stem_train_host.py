"""The training-mode stem restatement (tests/stem_train_restatement.py) on the host: the fixture's premises, the
restatement against the reference's stored maps, gradients and running buffers (tests/golden/stem_train_golden.npz:
torch on the CPU in float32, train()) within the float32-reference form of the bounds, a Richardson central difference
of the float64 loss, four mutants that each miss the fixture by a recorded factor, and the plan of
csrc/stem_train_plan.h under ASan + UBSan (tools/stem_train_plan_check.cpp: its own main, no preloading)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_io
import stem_train_restatement as st

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SRC = os.path.join(REPO, "tools", "stem_train_plan_check.cpp")
CASES = {"b2_12x20": (2, 12, 20), "b1_6x10": (1, 6, 10)}
MIN_FAR, MIN_COND = 1.1, 0.05  # tests/golden/gen_stem_train_golden.py
GRAD_KEYS = {"dx": "dx", "conv1.weight": "conv1.weight.grad", "bn1.weight": "bn1.weight.grad", "bn1.bias": "bn1.bias.grad"}


@functools.lru_cache(maxsize=None)
def fixture():
    return golden_io.load(GOLDEN, "stem_train_golden")


def params(g):
    return dict(conv1=g["conv1.weight"], bn1=tuple(g[f"bn1.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))


@functools.lru_cache(maxsize=None)
def case(name):
    g = fixture()
    p = params(g)
    c = {k: g[f"{name}/{k}"] for k in ("x", "z", "a", "pooled", "gp", "dx", "conv1.weight.grad", "bn1.weight.grad",
                                       "bn1.bias.grad", "running_mean_after", "running_var_after")}
    mean, var = st.tr.batch_stats(c["z"])
    c["stats"] = np.array([mean, var]).astype(np.float32)
    return p, c


def test_fixture_file_is_small_and_complete():
    path = os.path.join(GOLDEN, "stem_train_golden.npz")
    assert os.path.getsize(path) <= 256 << 10
    g = fixture()
    for name, (B, H, W) in CASES.items():
        oh, ow, ph, pw = st.sizes(H, W)
        assert g[f"{name}/x"].shape == (B, 3, H, W) and g[f"{name}/z"].shape == (B, oh, ow, 64)
        assert g[f"{name}/pooled"].shape == (B, ph, pw, 64) and int(g[f"{name}/num_batches_tracked"]) == 1


@pytest.mark.parametrize("name", CASES)
def test_fixture_premises(name):
    p, c = case(name)
    pre, lead, cond, far = st.premises(c["x"], p)
    print(f"{name}: smallest |pre-activation| {pre:.3e}, pool lead {lead:.3e}, var / mean z^2 >= {cond:.3f}, "
          f"running statistics >= {far:.2f} batch deviations away")
    assert pre >= st.MARGIN and lead >= st.MARGIN and cond >= MIN_COND and far >= MIN_FAR
    assert np.allclose([pre, lead, cond, far], fixture()[f"{name}/premises"], rtol=1e-9)
    # the stored float32 masks and window maxima are the float64 forward's
    V, _ = st.forward_chain(c["x"], p)
    assert np.array_equal(c["a"] > 0, V["pre"] > 0)
    assert np.array_equal(st.sr.pool_argmax(c["a"])[1], st.sr.pool_argmax(V["a"])[1])


@pytest.mark.parametrize("name", CASES)
def test_reference_inside_the_float32_bound(name):
    """Every element of the reference's z, a, pooled within the carried float32 forward bound; dx and the three
    parameter gradients within the float32-reference form of the bound of the restatement on the stored maps; the
    running buffers within the carried bound."""
    p, c = case(name)
    V, E32 = st.forward_chain(c["x"], p, f32=True)
    for k in ("z", "a", "pooled"):
        assert st.ratio(c[k], V[k], E32[k]) <= 1.0, k
    R, E = st.backward(c["x"], c, c["gp"], p, f32=True)
    d = {k: st.ratio(c[gk], R[k], E[k]) for k, gk in GRAD_KEYS.items()}
    print(name, "d_ref", " ".join(f"{k} {v:.4f}" for k, v in d.items()))
    assert max(d.values()) <= 1.0, d
    n = int(np.prod(c["z"].shape[:3]))
    for which, key in enumerate(("running_mean", "running_var")):
        before = p["bn1"][2 + which]
        r = st.running_update(before, V["stats"][which], n, which)
        b = st.running_bound(before, V["stats"][which], E32["stats"][which], n, which)
        assert st.ratio(c[key + "_after"], r, b) <= 1.0, key


@pytest.mark.parametrize("name", CASES)
def test_mutants_miss_the_fixture(name):
    """Running statistics in the forward, a biased variance in the running update, a dropped sum dY x^ term and the
    eval() gradient of the stem operator each miss the reference by more than 10 times the bound the true restatement
    meets."""
    p, c = case(name)
    V, E32 = st.forward_chain(c["x"], p, f32=True)
    Vr, _ = st.forward_chain(c["x"], p, f32=True, running=True)
    f_running = st.ratio(c["a"], Vr["a"], E32["a"])
    n = int(np.prod(c["z"].shape[:3]))
    before = p["bn1"][3]
    biased = (1.0 - st.MOMENTUM) * before.astype(np.float64) + st.MOMENTUM * V["stats"][1]
    f_biased = st.ratio(c["running_var_after"], biased, st.running_bound(before, V["stats"][1], E32["stats"][1], n, 1))
    R, E = st.backward(c["x"], c, c["gp"], p, f32=True)
    Rx, _ = st.backward(c["x"], c, c["gp"], p, f32=True, drop_xhat=True)
    f_xhat = max(st.ratio(c[GRAD_KEYS[k]], Rx[k], E[k]) for k in ("dx", "conv1.weight"))
    Re, _ = st.eval_backward(c["x"], c["a"], c["gp"], p, f32=True)
    f_eval = {k: st.ratio(c[gk], Re[k], E[k]) for k, gk in GRAD_KEYS.items()}
    print(f"{name}: mutants miss by running statistics {f_running:.3g}x, biased running variance {f_biased:.3g}x, "
          f"dropped x^ term {f_xhat:.3g}x, eval() gradient " + " ".join(f"{k} {v:.3g}x" for k, v in f_eval.items()))
    assert min(f_running, f_biased, f_xhat, max(f_eval.values())) > 10
    assert min(f_eval[k] for k in ("dx", "conv1.weight", "bn1.weight")) > 10


@pytest.mark.parametrize("shape", [(2, 6, 10), (1, 7, 9)])
def test_central_difference(shape):
    """L(t) = <gp, pooled(x + t d)> differentiated at t = 0 in float64.  t keeps every pre-activation's sign and every
    window's first maximum (asserted), so L is smooth on [-t, t] but not a polynomial: the central differences at t,
    t / 2, t / 4 are Richardson-extrapolated twice, and what the last extrapolation moved is taken as its truncation.
    Rounding: a term of L passes through at most n = 147 + 3 npix + 24 float64 roundings, so a difference quotient at
    step t / 4 errs by n 2^-53 S_L / (t / 4), weight 64 / 45 in the extrapolation (8 covers it)."""
    p = st.draw_params(3)
    x, gp = st.draw_case(*shape, 5)
    x, gp = x.astype(np.float64), gp.astype(np.float64)
    V, _ = st.forward_chain(x, p)
    arg = st.sr.pool_argmax(V["a"])[1]
    R, _ = st.backward(x, dict(z=V["z"], a=V["a"], stats=V["stats"]), gp, p)
    d = np.random.default_rng(9).standard_normal(x.shape)
    h0 = 1e-6
    Vp, Vm = st.forward_chain(x + h0 * d, p)[0], st.forward_chain(x - h0 * d, p)[0]
    slope = np.maximum(np.abs(Vp["pre"] - Vm["pre"]) / (2 * h0), 1e-300)
    t = 0.25 * min(float(np.min(np.abs(V["pre"]) / slope)), st.pool_lead(V["a"]) / (2 * float(slope.max())))
    assert t > 1e-9
    for sign in (-1.0, 1.0):
        Vt = st.forward_chain(x + sign * t * d, p)[0]
        assert np.array_equal(Vt["pre"] > 0, V["pre"] > 0) and np.array_equal(st.sr.pool_argmax(Vt["a"])[1], arg)
    L = lambda v: float((st.forward_chain(v, p)[0]["pooled"] * gp).sum())  # noqa: E731
    fd = [(L(x + (t / k) * d) - L(x - (t / k) * d)) / (2 * t / k) for k in (1, 2, 4)]
    r1 = [(4 * fd[1] - fd[0]) / 3, (4 * fd[2] - fd[1]) / 3]
    r2 = (16 * r1[1] - r1[0]) / 15
    exact = float((R["dx"] * d).sum())
    npix = int(np.prod(V["z"].shape[:3]))
    n = st.K + 3 * npix + 24
    S_L = float((np.abs(gp) * (2 * np.abs(V["pooled"]) + 1.0)).sum())
    tol = abs(r2 - r1[1]) + 8 * n * st.U53 * S_L / t + (n + x.size) * st.U53 * float((np.abs(R["dx"]) * np.abs(d)).sum())
    print(f"{shape}: finite difference {r2:.12g}, restatement {exact:.12g}, tolerance {tol:.3e}")
    assert abs(r2 - exact) <= tol, (r2, exact, t, tol)


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    """tools/stem_train_plan_check built with the host sanitizers, once for the module."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stem_train") / "stem_train_plan_check")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_plan_check_under_host_sanitizers(helper):
    r = subprocess.run([helper], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and " plans, 0 bad" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
