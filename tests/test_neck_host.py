"""The FPN neck operator on the host: the numpy float64 restatement (tests/neck_restatement.py) against the reference's
stored outputs and gradients (tests/golden/neck_golden*.npz), finite differences, the adjoint identity of the resize,
one-hot known answers, and the stand-alone plan check under ASan + UBSan (tools/neck_plan_check.cpp: its own main,
no preloading)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import golden_io
import neck_restatement as nr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SRC = os.path.join(REPO, "tools", "neck_plan_check.cpp")
PNAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
GRADS = ("d_l1", "d_l2", "d_l3", "d_l4", "dW1", "db1", "dW2", "db2", "dW3", "db3")


@pytest.fixture(scope="module")
def golden():
    return golden_io.load(GOLDEN, "neck_golden")


def test_fixture_files_are_small_and_complete(golden):
    files = [f for f in os.listdir(GOLDEN) if f.startswith("neck_golden") and f.endswith(".npz")]
    assert files and all(os.path.getsize(os.path.join(GOLDEN, f)) <= golden_io.MAX_FILE_BYTES for f in files)
    assert list(golden["cases"]) == ["B2_1x1", "B2_2x3", "B2_3x2"]
    assert [golden[k].shape for k in PNAMES] == [(256, 768), (256,), (128, 384), (128,), (64, 192), (64,)]
    for p, q in zip(nr.draw_params(7), (golden[k] for k in PNAMES)):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("name", ["B2_1x1", "B2_2x3", "B2_3x2"])
def test_reference_inside_twice_the_bound(golden, name):
    """The reference (torch on the CPU, float32) against the restatement: inside the kernels' bound doubled for the
    reference's own float32 rounding, with the f32 variant of the bound where the reference also sums in float32
    what the kernels sum in float64 (U^T and the bias gradients: neck_restatement.backward)."""
    g = golden
    params = [g[k] for k in PNAMES]
    ls = [g[f"{name}/l{i}"] for i in (1, 2, 3, 4)]
    gs = [g[f"{name}/g{i}"] for i in (2, 3, 4)]
    us, Ef = nr.forward(*ls, params)
    worst = {}
    for k, r, e in zip(("u2", "u3", "u4"), us, Ef):
        worst[k] = float(np.max(np.abs(g[f"{name}/{k}"] - r) / (2 * e)))
    R, E, _ = nr.backward(*ls, g[f"{name}/u2"], g[f"{name}/u3"], *gs, params, f32=True)
    for k in GRADS:
        assert g[f"{name}/{k}"].shape == R[k].shape
        worst[k] = float(np.max(np.abs(g[f"{name}/{k}"] - R[k]) / (2 * E[k])))
    print(name, {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert np.allclose(2 * max(worst.values()), np.max(g[f"{name}/d_ref"]))  # what the generator recorded


def test_central_differences_are_exact_to_rounding():
    """<u2, g2> + <u3, g3> + <u4, g4> is linear in the four maps and affine in each parameter tensor alone, so a
    central difference along any direction in one of those groups is the directional derivative up to float64
    rounding."""
    rng = np.random.default_rng(3)
    ls, gs = nr.draw_case(1, 2, 3, 17)
    params = nr.draw_params(5)
    (u2, u3, _), _ = nr.forward(*ls, params)
    R, _, _ = nr.backward(*ls, u2, u3, *gs, params)
    ls64 = [a.astype(np.float64) for a in ls]
    p64 = [a.astype(np.float64) for a in params]
    scale = abs(nr.loss(*ls64, p64, *gs)) + 1.0
    dirs = [rng.standard_normal(a.shape) for a in ls64]
    eps = 0.5
    fd = (nr.loss(*[a + eps * d for a, d in zip(ls64, dirs)], p64, *gs)
          - nr.loss(*[a - eps * d for a, d in zip(ls64, dirs)], p64, *gs)) / (2 * eps)
    an = sum(float((R[f"d_l{i + 1}"] * dirs[i]).sum()) for i in range(4))
    assert abs(fd - an) <= 1e-10 * max(scale, abs(an)), (fd, an)
    for j, k in enumerate(("dW1", "db1", "dW2", "db2", "dW3", "db3")):
        d = rng.standard_normal(p64[j].shape)
        plus = [a + eps * d if i == j else a for i, a in enumerate(p64)]
        minus = [a - eps * d if i == j else a for i, a in enumerate(p64)]
        fd = (nr.loss(*ls64, plus, *gs) - nr.loss(*ls64, minus, *gs)) / (2 * eps)
        an = float((R[k] * d).sum())
        assert abs(fd - an) <= 1e-10 * max(scale, abs(an)), (k, fd, an)


@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 3), (19, 19), (1, 5), (4, 1), (3, 7)])
def test_adjoint_identity(hw):
    h, w = hw
    rng = np.random.default_rng(h * 100 + w)
    a = rng.standard_normal((2, h, w, 3))
    b = rng.standard_normal((2, 2 * h, 2 * w, 3))
    lhs, rhs = float((nr.up(a) * b).sum()), float((a * nr.up_t(b)).sum())
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(nr.up(np.abs(a)) * np.abs(b)).sum() + 1.0)
    # rows of U sum to 1 up to the float32 rounding of l0 = 1 - l1, and every coefficient is in [0, 1]
    for n in (h, w):
        M = nr.up_matrix(n)
        assert M.min() >= 0.0 and M.max() <= 1.0 and np.all(np.abs(M.sum(1) - 1.0) <= 2.0 ** -23)
        assert np.all((M != 0).sum(0) <= 5)  # a source is reached by at most 5 outputs per axis


def test_resize_matches_torch():
    rng = np.random.default_rng(0)
    for h, w in ((1, 1), (2, 3), (19, 19), (1, 4)):
        x = rng.standard_normal((1, h, w, 2)).astype(np.float32)
        want = torch.nn.functional.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2).double(), scale_factor=2,
                                               mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
        # float32 coefficients: scale and scale * o are each rounded once, so a source index f < n is off by at most
        # 2 u n, and a weight error d moves one axis' interpolation by at most 2 d max|x|
        assert np.max(np.abs(nr.up(x) - want)) <= 2 * 2 * (2 * 2.0 ** -24 * max(h, w)) * np.abs(x).max()


def test_one_hot_known_answers():
    params = nr.draw_params(9)
    W1, _, W2, _, W3, _ = params
    ls, _ = nr.draw_case(1, 2, 3, 4)
    (u2, u3, _), _ = nr.forward(*ls, params)
    B, H, W = 1, 16, 24
    # g4 one-hot at (p, o): d_l1[p, :] = W3[o, 128:], nothing elsewhere
    g4 = np.zeros((B, H, W, 64), np.float32)
    g4[0, 5, 7, 11] = 1.0
    R, _, _ = nr.backward(*ls, u2, u3, None, None, g4, params)
    want = np.zeros((B, H, W, 64))
    want[0, 5, 7] = W3[11, 128:]
    assert np.array_equal(R["d_l1"], want)
    # g3 one-hot: dZ2 holds exactly the four forward coefficients of that output pixel
    for y, x in ((5, 7), (0, 0), (15, 23), (8, 1)):
        g3 = np.zeros((B, H, W, 128), np.float32)
        g3[0, y, x, 3] = 1.0
        _, _, mid = nr.backward(*ls, u2, u3, None, g3, np.zeros_like(g4), params)
        y0, y1, ly0, ly1 = (v[y] for v in nr.up_coeffs(H // 2))
        x0, x1, lx0, lx1 = (v[x] for v in nr.up_coeffs(W // 2))
        want = np.zeros((B, H // 2, W // 2, 128))
        for yy, cy in ((y0, ly0), (y1, ly1)):
            for xx, cx in ((x0, lx0), (x1, lx1)):
                want[0, yy, xx, 3] += float(cy) * float(cx)
        assert np.array_equal(mid["dZ2"], want) and np.count_nonzero(want) <= 4
    # h = 1 / w = 1: scale 0, both outputs take the single source with weight 1
    assert np.array_equal(nr.up_matrix(1), [[1.0], [1.0]])
    i0, i1, l0, l1 = nr.up_coeffs(1)
    assert list(i0) == [0, 0] and list(i1) == [0, 0] and list(l0) == [1, 1] and list(l1) == [0, 0]
    g = np.arange(2 * 2 * 6 * 1, dtype=np.float64).reshape(1, 2, 6, 2)[..., :1]
    assert np.allclose(nr.up_t(g)[0, 0, :, 0], nr.up_matrix(3).T @ g[0].sum(0)[:, 0], rtol=1e-14, atol=0)


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    """tools/neck_plan_check built with the host sanitizers, once for the module."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("neck") / "neck_plan_check")
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
