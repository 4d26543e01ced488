"""The training-mode BasicBlock restatement (tests/block_train_restatement.py) on the host: the fixture's premises,
the restatement against the reference's stored gradients, y and running buffers (tests/golden/block_train_golden*.npz:
torch on the CPU in float32, train()) within the float32-reference form of the bounds, a Richardson central difference
of the float64 loss, the identities sum dZ = 0 and sum dZ (z - mean) = 0, the running-buffer update against
nn.BatchNorm2d, three mutants that each miss the fixture by a recorded factor, the device's one-pass variance formula
inside its bound, and the plan of csrc/block_train_plan.h under ASan + UBSan (tools/block_train_plan_check.cpp: its
own main, no preloading)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import block_train_restatement as tr
import golden_io

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SRC = os.path.join(REPO, "tools", "block_train_plan_check.cpp")
FIXTURE = [(1, 0, (2, 3, 5)), (2, 0, (2, 5, 7)), (2, 0, (1, 4, 6))]
MIN_COND, MIN_FAR = 0.05, 1.0  # tests/golden/gen_block_train_golden.py


def _name(layer, block, shape):
    return f"L{layer}b{block}_B{shape[0]}_{shape[1]}x{shape[2]}"


@functools.lru_cache(maxsize=None)
def fixture():
    return golden_io.load(GOLDEN, "block_train_golden")


@functools.lru_cache(maxsize=None)
def case(name):
    g = fixture()
    layer, block = int(g[f"{name}/layer"]), int(g[f"{name}/block"])
    _, _, s, ds = tr.block_shape(layer, block)
    p = tr.fixture_params(g, layer, block)
    maps = {k: g[f"{name}/{k}"] for k in ["z1", "mid", "z2", "y", "stats"] + (["zd"] if ds else [])}
    keys = ["dx"] + list(tr.PARAMS[:9 if ds else 6])
    return layer, block, s, ds, p, g[f"{name}/x"], g[f"{name}/gy"], maps, keys


def test_fixture_files_are_small_and_complete():
    files = [f for f in os.listdir(GOLDEN) if f.startswith("block_train_golden") and f.endswith(".npz")]
    assert files and all(os.path.getsize(os.path.join(GOLDEN, f)) <= golden_io.MAX_FILE_BYTES for f in files)
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in files) <= 4 << 20
    assert list(fixture()["cases"]) == [_name(*c) for c in FIXTURE]


@pytest.mark.parametrize("layer,block,shape", FIXTURE)
def test_fixture_premises(layer, block, shape):
    name = _name(layer, block, shape)
    g = fixture()
    _, _, s, ds, p, x, gy, maps, _ = case(name)
    assert len(tr.param_list(p)) == (9 if ds else 6) and all(a.dtype == np.float32 for a in tr.param_list(p))
    dx, dgy = tr.draw_x(layer, block, *shape, int(g[f"{name}/seed"]))
    assert np.array_equal(dx, x) and np.array_equal(dgy, gy)
    margin, worst, cond, far = tr.premises(x, p, s)
    print(f"{name}: smallest |pre-activation| {margin:.3e}, worst carried bound {worst:.3e}, var / mean z^2 >= {cond:.3f}, "
          f"running statistics >= {far:.2f} batch deviations away")
    assert margin >= tr.MARGIN and cond >= MIN_COND and far >= MIN_FAR
    # the stored float32 masks are the float64 forward's
    V, _ = tr.forward_chain(x, p, s)
    assert np.array_equal(maps["mid"] > 0, V["pre1"] > 0) and np.array_equal(maps["y"] > 0, V["pre2"] > 0)
    # the stored statistics are the two-pass float64 ones of the stored z, rounded once
    for i, zk in enumerate(["z1", "z2"] + (["zd"] if ds else [])):
        mean, var = tr.batch_stats(maps[zk])
        assert np.array_equal(maps["stats"][i], np.array([mean, var]).astype(np.float32))
    assert int(g[f"{name}/num_batches_tracked"]) == 1


@pytest.mark.parametrize("layer,block,shape", FIXTURE)
def test_reference_inside_the_float32_bound(layer, block, shape):
    """Every element of the reference's dx and 6 or 9 parameter gradients within the float32-reference form of the
    bound of the restatement on the stored maps; y and the running buffers within the carried forward bound."""
    name = _name(layer, block, shape)
    g = fixture()
    _, _, s, ds, p, x, gy, maps, keys = case(name)
    R, E = tr.backward(x, maps, gy, p, s, f32=True)
    d = [tr.ratio(g[f"{name}/{k}"], R[k], E[k]) for k in keys]
    print(name, "d_ref", " ".join(f"{k} {v:.4f}" for k, v in zip(keys, d)))
    assert max(d) <= 1.0, dict(zip(keys, d))
    assert np.allclose(d, g[f"{name}/d_ref"], rtol=1e-6, atol=0), "d_ref does not describe the stored data"
    V, E32 = tr.forward_chain(x, p, s, f32=True)
    for k in ["z1", "mid", "z2", "y"] + (["zd"] if ds else []):
        assert tr.ratio(maps[k], V[k], E32[k]) <= 1.0, k
    n = int(np.prod(gy.shape[:3]))
    before, after = g[f"{name}/running_before"], g[f"{name}/running_after"]
    for i in range(before.shape[0]):
        for which in (0, 1):
            r = tr.running_update(before[i, which], V["stats"][i, which], n, which)
            b = tr.running_bound(before[i, which], V["stats"][i, which], E32["stats"][i, which], n, which)
            assert tr.ratio(after[i, which], r, b) <= 1.0, (i, which)


@pytest.mark.parametrize("layer,block,shape", FIXTURE[:2])
def test_mutants_miss_the_fixture(layer, block, shape):
    """Running statistics in the forward, a biased variance in the running update and a dropped sum dY x^ term in dZ
    each miss the reference by a large factor of the bound the true restatement meets."""
    name = _name(layer, block, shape)
    g = fixture()
    _, _, s, ds, p, x, gy, maps, keys = case(name)
    V, E32 = tr.forward_chain(x, p, s, f32=True)
    # 1. running statistics: the eval() forward
    x64 = x.astype(np.float64)
    c1 = tr.coef(p["bn1"][0], p["bn1"][1], p["bn1"][2], p["bn1"][3])
    mid = np.maximum(c1[0] * tr.conv_stage(x64, p["conv1"], s)[0] + c1[1], 0.0)
    c2 = tr.coef(p["bn2"][0], p["bn2"][1], p["bn2"][2], p["bn2"][3])
    v = c2[0] * tr.conv_stage(mid, p["conv2"], 1)[0] + c2[1]
    if ds:
        cd = tr.coef(p["bnd"][0], p["bnd"][1], p["bnd"][2], p["bnd"][3])
        v = v + cd[0] * tr.conv_stage(x64, p["convd"], s)[0] + cd[1]
    else:
        v = v + x64
    f_running = tr.ratio(g[f"{name}/y"], np.maximum(v, 0.0), E32["y"])
    # 2. a biased variance in the running update
    n = int(np.prod(gy.shape[:3]))
    before, after = g[f"{name}/running_before"], g[f"{name}/running_after"]
    biased = (1.0 - tr.MOMENTUM) * before[0, 1].astype(np.float64) + tr.MOMENTUM * V["stats"][0, 1]
    f_biased = tr.ratio(after[0, 1], biased, tr.running_bound(before[0, 1], V["stats"][0, 1], E32["stats"][0, 1], n, 1))
    # 3. dZ without its sum dY (z - mean) term
    R, E = tr.backward(x, maps, gy, p, s, f32=True, drop_xhat=True)
    f_xhat = max(tr.ratio(g[f"{name}/{k}"], R[k], E[k]) for k in ("dx", "conv1.weight", "conv2.weight"))
    print(f"{name}: mutants miss by running statistics {f_running:.3g}x, biased running variance {f_biased:.3g}x, "
          f"dropped x^ term {f_xhat:.3g}x of the bound")
    assert min(f_running, f_biased, f_xhat) > 10


@pytest.mark.parametrize("layer,block,shape", [(1, 1, (2, 3, 4)), (2, 0, (2, 5, 4))])
def test_identities_and_central_difference(layer, block, shape):
    """sum_p dZ = 0 and sum_p dZ (z - mean) = 0 per channel for every BatchNorm (the gradient of a function that does
    not change when z is shifted and, for eps = 0, scaled: with eps the second sum is gamma invstd^3 eps Bq), to float64
    rounding of the sums' absolute terms; and L(t) = <gy, y(x + t d)>
    differentiated at t = 0.  t keeps every pre-activation's sign (a quarter of the smallest |pre| / |d pre / dt|), so L
    is smooth on [-t, t] but, unlike the eval() block's, not a polynomial: the central differences at t, t / 2, t / 4
    are Richardson-extrapolated twice (truncation O(t^6)), and what the last extrapolation moved is taken as 15 times
    its own truncation.  Rounding: a term of L passes through at most n = K1 + K2 + 3 npix + 24 float64 roundings, so
    a difference quotient at step t / 4 errs by n 2^-53 S_L / (t / 4), weight 64 / 45 in the extrapolation."""
    _, _, s, ds = tr.block_shape(layer, block)
    p = tr.draw_params(layer, block, 3)
    x, gy = tr.draw_x(layer, block, *shape, 5)
    x, gy = x.astype(np.float64), gy.astype(np.float64)
    V, _ = tr.forward_chain(x, p, s)
    maps = {k: V[k] for k in ("z1", "mid", "z2", "y", "stats")}
    maps["zd"] = V.get("zd")
    R, _ = tr.backward(x, maps, gy, p, s)
    for i, (bn, zk) in enumerate(zip(tr.BNS, ("z1", "z2", "zd"))):
        if bn not in R["_dZ"]:
            continue
        dZ, z = tr._flat(R["_dZ"][bn]), tr._flat(V[zk])
        xc = z - V["stats"][i, 0]
        assert np.all(np.abs(dZ.sum(0)) <= 64 * dZ.shape[0] * tr.U53 * np.abs(dZ).sum(0) + 1e-300)
        # with eps > 0 the second identity is exact as sum dZ (z - mean) = gamma invstd^3 eps Bq (var / (var + eps) < 1)
        gam, var = np.asarray(p[bn][0], np.float64), V["stats"][i, 1]
        rest = gam * (var + tr.EPS) ** -1.5 * tr.EPS * (tr._flat(R["_dY"][bn]) * xc).sum(0)
        assert np.all(np.abs((dZ * xc).sum(0) - rest) <= 64 * dZ.shape[0] * tr.U53 * (np.abs(dZ) * np.abs(xc)).sum(0) + 1e-300)
    d = np.random.default_rng(9).standard_normal(x.shape)
    h0 = 1e-6
    Vp, Vm = tr.forward_chain(x + h0 * d, p, s)[0], tr.forward_chain(x - h0 * d, p, s)[0]
    t = 0.25 * min(float(np.min(np.abs(V[k]) / np.maximum(np.abs(Vp[k] - Vm[k]) / (2 * h0), 1e-300))) for k in ("pre1", "pre2"))
    assert t > 1e-9
    for sign in (-1.0, 1.0):
        Vt = tr.forward_chain(x + sign * t * d, p, s)[0]
        assert np.array_equal(Vt["pre1"] > 0, V["pre1"] > 0) and np.array_equal(Vt["pre2"] > 0, V["pre2"] > 0)
    L = lambda v: float((tr.forward_chain(v, p, s)[0]["y"] * gy).sum())  # noqa: E731
    fd = [(L(x + (t / k) * d) - L(x - (t / k) * d)) / (2 * t / k) for k in (1, 2, 4)]
    r1 = [(4 * fd[1] - fd[0]) / 3, (4 * fd[2] - fd[1]) / 3]
    r2 = (16 * r1[1] - r1[0]) / 15
    exact = float((R["dx"] * d).sum())
    npix = int(np.prod(gy.shape[:3]))
    n = 9 * x.shape[3] + 9 * gy.shape[3] + 3 * npix + 24
    S_L = float((np.abs(gy) * (np.abs(V["pre2"]) + 2 * np.abs(V["y"]) + 1.0)).sum())
    tol = abs(r2 - r1[1]) + 8 * n * tr.U53 * S_L / t + (n + x.size) * tr.U53 * float((np.abs(R["dx"]) * np.abs(d)).sum())
    print(f"layer{layer}.{block}: finite difference {r2:.12g}, restatement {exact:.12g}, tolerance {tol:.3e}")
    assert abs(r2 - exact) <= tol, (r2, exact, t, tol)


def test_one_pass_variance_inside_its_bound():
    """The device's var = max(S2 / n - mean^2, 0) in float64 against the two-pass value, a large mean included."""
    rng = np.random.default_rng(1)
    for n, shift in ((2, 0.0), (30, 0.3), (70, 5.0), (4096, 40.0)):
        z = (rng.standard_normal((n, 8)) + shift).astype(np.float32)
        (mean, var), (Em, Ev) = tr.stats_stage(z)
        m1, v1 = tr.batch_stats_one_pass(z)
        assert np.all(np.abs(m1 - mean) <= Em) and np.all(np.abs(v1 - var) <= Ev)
        assert np.all(np.abs(m1.astype(np.float32) - mean) <= Em) and np.all(np.abs(v1.astype(np.float32) - var) <= Ev)


@pytest.mark.parametrize("n,momentum", [(2, 0.1), (30, 0.1), (6, 0.5)])
def test_running_update_against_batchnorm2d(n, momentum):
    rng = np.random.default_rng(n)
    z = rng.standard_normal((n, 4))
    bn = torch.nn.BatchNorm2d(4, momentum=momentum).double().train()
    before = (rng.standard_normal(4) + 3.0, rng.uniform(4.0, 9.0, 4))
    bn.running_mean.copy_(torch.from_numpy(before[0]))
    bn.running_var.copy_(torch.from_numpy(before[1]))
    bn(torch.from_numpy(z.T.reshape(1, 4, n, 1).copy()))
    mean, var = tr.batch_stats(z)
    for which, (buf, stat) in enumerate(((bn.running_mean, mean), (bn.running_var, var))):
        got = tr.running_update(before[which], stat, n, which, momentum)
        assert np.max(np.abs(got - buf.numpy())) <= 1e-13 * np.max(np.abs(got))
    assert int(bn.num_batches_tracked) == 1


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    """tools/block_train_plan_check built with the host sanitizers, once for the module."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("block_train") / "block_train_plan_check")
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
