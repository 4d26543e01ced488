"""The stem's restatement (tests/stem_restatement.py) on the host: against the reference fixture
(tests/golden/stem_golden.npz: torch on the CPU in float32, the stem not folded) within the sum of both bounds, against
a central finite difference of the float64 loss, the adjoint identity of the data gradient, known answers of the pool
adjoint's first-maximum rule, and the plan of csrc/stem_grad_plan.h under ASan + UBSan (tools/stem_grad_plan_check.cpp:
its own main, no preloading)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_io
import stem_restatement as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SRC = os.path.join(REPO, "tools", "stem_grad_plan_check.cpp")
CASES = ("b2_12x20", "b1_6x10")
PARAMS = ("conv1.weight", "bn1.weight", "bn1.bias")


@functools.lru_cache(maxsize=None)
def fixture():
    return golden_io.load(GOLDEN, "stem_golden")


def fixture_params():
    g = fixture()
    return dict(conv1=g["conv1.weight"], bn1=tuple(g[f"bn1.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))


def nhwc(t):
    return np.ascontiguousarray(np.transpose(t, (0, 2, 3, 1)))


@functools.lru_cache(maxsize=None)
def reference_case(case):
    """The fixture's case as the restatement takes it, with the restatement's own gradients on the fixture's a in both
    arithmetic forms: (maps, (R, E) in the GPU's form at K_c = all pixels, (R, E32) in the reference's form)."""
    g, p = fixture(), fixture_params()
    m = dict(x=g[f"{case}/x"], a=nhwc(g[f"{case}/a"]), pooled=nhwc(g[f"{case}/pooled"]), gp=nhwc(g[f"{case}/gp"]))
    return m, sr.unfolded(p, m["x"], m["a"], m["gp"]), sr.unfolded(p, m["x"], m["a"], m["gp"], f32=True)


@pytest.mark.parametrize("case", CASES)
def test_fixture_premises(case):
    g, p = fixture(), fixture_params()
    x = g[f"{case}/x"]
    assert sr.margins(p, x) >= sr.MARGIN
    B, _, H, W = x.shape
    oh, ow, ph, pw = sr.sizes(H, W)
    assert g[f"{case}/a"].shape == (B, 64, oh, ow) and g[f"{case}/pooled"].shape == (B, 64, ph, pw)
    assert np.count_nonzero(g[f"{case}/dx"]) and np.count_nonzero(g[f"{case}/gp"] == 0)


@pytest.mark.parametrize("case", CASES)
def test_restatement_forward_matches_the_reference(case):
    g, p = fixture(), fixture_params()
    Wf, bf = sr.fold(p)
    a, pooled = sr.forward(g[f"{case}/x"], Wf, bf)
    # 147-term float32 dot products on either side plus the fold's roundings, relative to the sum of absolute terms
    S = sr.patches(np.abs(g[f"{case}/x"])) @ np.abs(Wf.astype(np.float64)).reshape(64, 147).T + np.abs(bf)
    bound = (147 + 2 + sr.br.REF_EXTRA) * sr.U24 * S
    assert np.all(np.abs(a - nhwc(g[f"{case}/a"])) <= bound)
    assert np.all(np.abs(pooled - nhwc(g[f"{case}/pooled"])) <= sr.pool_argmax(bound)[0])
    assert np.array_equal(sr.pool_argmax(nhwc(g[f"{case}/a"]))[0], nhwc(g[f"{case}/pooled"]).astype(np.float64))


@pytest.mark.parametrize("case", CASES)
def test_restatement_gradients_match_the_reference(case):
    g = fixture()
    _, (R, E), (_, E32) = reference_case(case)
    for k, name in (("dx", "dx"),) + tuple((n, n + ".grad") for n in PARAMS):
        q = sr.ratio(g[f"{case}/{name}"], R[k], E[k] + E32[k])
        print(f"{case} {k}: error / bound {q:.3f}")
        assert q <= 1.0, k


def test_central_finite_difference():
    p = sr.draw_params(5)
    Wf, bf = sr.fold(p)
    rng = np.random.default_rng(6)
    x = sr.condition_image(p, rng.standard_normal((1, 3, 6, 10)).astype(np.float32)).astype(np.float64)
    gp = rng.standard_normal((1, 2, 3, 64))

    def loss(x_, W_, b_):
        return float((sr.forward(x_, W_, b_)[1] * gp).sum())

    a, _ = sr.forward(x, Wf, bf)
    R, _ = sr.backward(x, a, gp, Wf)
    h = 1e-6  # far below the conditioned margin: no branch changes
    Wd, bd = Wf.astype(np.float64), bf.astype(np.float64)
    for _ in range(24):
        i = tuple(int(rng.integers(0, n)) for n in x.shape)
        e = np.zeros_like(x)
        e[i] = h
        fd = (loss(x + e, Wd, bd) - loss(x - e, Wd, bd)) / (2 * h)
        assert abs(fd - R["dx"][i]) <= 1e-6 * max(1.0, abs(fd)), i
        j = tuple(int(rng.integers(0, n)) for n in Wd.shape)
        e = np.zeros_like(Wd)
        e[j] = h
        fd = (loss(x, Wd + e, bd) - loss(x, Wd - e, bd)) / (2 * h)
        assert abs(fd - R["dW"][j]) <= 1e-6 * max(1.0, abs(fd)), j
    for o in range(0, 64, 7):
        e = np.zeros_like(bd)
        e[o] = h
        fd = (loss(x, Wd, bd + e) - loss(x, Wd, bd - e)) / (2 * h)
        assert abs(fd - R["db"][o]) <= 1e-6 * max(1.0, abs(fd)), o


@pytest.mark.parametrize("H,W", [(6, 10), (7, 9), (12, 20)])
def test_adjoint_identity(H, W):
    rng = np.random.default_rng(H * 100 + W)
    Wf = rng.standard_normal((64, 3, 7, 7))
    x = rng.standard_normal((2, 3, H, W))
    oh, ow, _, _ = sr.sizes(H, W)
    dA = rng.standard_normal((2, oh, ow, 64))
    lhs, rhs = float((sr.dgrad7(dA, Wf, H, W) * x).sum()), float((dA * sr.conv7(x, Wf)).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), 1.0)


def pool_known_answers():
    """[(name, a (1, oh, ow, 64), gp, expected dA)]: one-hot cases of the first-maximum rule, the same in every channel."""
    out = []

    def case(name, a2, gp2, want2):
        a = np.repeat(np.asarray(a2, np.float32)[None, :, :, None], 64, 3)
        gp = np.repeat(np.asarray(gp2, np.float32)[None, :, :, None], 64, 3)
        out.append((name, a, gp, np.repeat(np.asarray(want2, np.float32)[None, :, :, None], 64, 3)))

    # window (1, 1) of a 4 x 4 map covers rows 1..3, columns 1..3: two equal positive maxima at (1, 2) and (2, 1);
    # (1, 2) comes first in the row-major scan and takes everything
    a = np.zeros((4, 4))
    a[1, 2] = a[2, 1] = 5.0
    gp = np.zeros((2, 2))
    gp[1, 1] = 3.0
    want = np.zeros((4, 4))
    want[1, 2] = 3.0
    case("tie", a, gp, want)
    # all-zero windows send nothing anywhere, whatever gp holds
    case("zeros", np.zeros((4, 4)), np.full((2, 2), 7.0), np.zeros((4, 4)))
    # window (0, 0) covers rows -1..1, columns -1..1: the padding is ignored, the only positive cell (1, 1) wins; on
    # the odd 3 x 5 map window (1, 2) reads a row and a column of padding and its winner is the corner (2, 4)
    a = np.zeros((3, 5))
    a[1, 1] = 2.0
    a[2, 4] = 1.0
    gp = np.zeros((2, 3))
    gp[0, 0] = 4.0
    gp[1, 2] = 6.0
    want = np.zeros((3, 5))
    want[1, 1] = 4.0
    want[2, 4] = 6.0
    case("border", a, gp, want)
    # one cell that is the first maximum of all four windows holding it collects all four
    a = np.zeros((4, 4))
    a[1, 1] = 1.0
    want = np.zeros((4, 4))
    want[1, 1] = 1.0 + 2.0 + 3.0 + 4.0
    case("four", a, [[1.0, 2.0], [3.0, 4.0]], want)
    return out


@pytest.mark.parametrize("name,a,gp,want", pool_known_answers(), ids=lambda v: v if isinstance(v, str) else "")
def test_pool_adjoint_known_answers(name, a, gp, want):
    dap, _ = sr.pool_adjoint(a, gp)
    assert np.array_equal(np.where(a > 0, dap, 0.0), want.astype(np.float64))


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    """tools/stem_grad_plan_check built with the host sanitizers, once for the module."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stem") / "stem_grad_plan_check")
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
