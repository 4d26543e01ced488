"""The BasicBlock restatement (tests/block_restatement.py) on the CPU: against the reference's stored gradients
(tests/golden/block_golden*.npz) and against torch's float64 autograd of the block in eval(), both element by element
within the float32-reference form of the derived bound,
a central finite difference, the adjoint identity at both strides, the BatchNorm unfold against torch autograd, and
one-hot known answers of the stride-2 data gradient."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_restatement as br
import golden_io


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _torch_block(p, x_nhwc, s):
    """The block in eval() under torch autograd in float64 on the float32 parameters: (leaves, mid, y)."""
    leaves = {}

    def leaf(name, a):
        leaves[name] = _t(a).requires_grad_(True)
        return leaves[name]

    def bn(v, key):
        g, b, mu, var = p[key]
        return F.batch_norm(v, _t(mu), _t(var), leaf(key + ".g", g), leaf(key + ".b", b), False, 0.1, br.EPS)

    x = leaf("x", np.asarray(x_nhwc).transpose(0, 3, 1, 2))
    mid = F.relu(bn(F.conv2d(x, leaf("conv1", p["conv1"]), stride=s, padding=1), "bn1"))
    z = bn(F.conv2d(mid, leaf("conv2", p["conv2"]), padding=1), "bn2")
    skip = bn(F.conv2d(x, leaf("convd", p["convd"]), stride=s), "bnd") if "convd" in p else x
    return leaves, mid, F.relu(z + skip)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = [(1, 0, (2, 3, 5)), (2, 0, (2, 5, 7)), (2, 0, (1, 4, 6))]
KEYS = ("dx", "conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "convd.weight",
        "bnd.weight", "bnd.bias")


@pytest.fixture(scope="module")
def golden():
    return golden_io.load(GOLDEN, "block_golden")


def _name(layer, block, shape):
    return f"L{layer}b{block}_B{shape[0]}_{shape[1]}x{shape[2]}"


def test_fixture_files_are_small_and_complete(golden):
    files = [f for f in os.listdir(GOLDEN) if f.startswith("block_golden") and f.endswith(".npz")]
    assert files and all(os.path.getsize(os.path.join(GOLDEN, f)) <= golden_io.MAX_FILE_BYTES for f in files)
    assert sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in files) <= 4 << 20
    assert list(golden["cases"]) == [_name(*c) for c in FIXTURE]


@pytest.mark.parametrize("layer,block,shape", FIXTURE)
def test_reference_inside_the_float32_bound(golden, layer, block, shape):
    """The reference's BasicBlock (torch on the CPU, float32, eval()) against the restatement on the stored maps:
    every element of dx and of the 6 or 9 parameter gradients within the float32-reference form of the bound."""
    c = _name(layer, block, shape)
    assert (int(golden[f"{c}/layer"]), int(golden[f"{c}/block"])) == (layer, block)
    p = br.draw_params(layer, block, int(golden[f"{c}/param_seed"]))
    drawn = br.draw_case(layer, block, *shape, int(golden[f"{c}/seed"]))
    assert np.array_equal(drawn["x"], golden[f"{c}/x"]) and np.array_equal(drawn["gy"], golden[f"{c}/gy"])
    maps = {k: golden[f"{c}/{k}"] for k in ("x", "mid", "y", "gy")}
    R, E = br.unfolded(layer, block, p, maps, f32=True)
    keys = [k for k in KEYS if k in R]
    assert len(keys) == (10 if "convd" in p else 7)
    d = [br.ratio(golden[f"{c}/{k}"], R[k], E[k]) for k in keys]
    print(c, "d_ref", " ".join(f"{k} {v:.4f}" for k, v in zip(keys, d)))
    assert max(d) <= 1.0, dict(zip(keys, d))
    assert np.allclose(d, golden[f"{c}/d_ref"], rtol=1e-6, atol=0), "d_ref does not describe the stored data"
    # the stored mid and y are the restatement's forward within the float32-reference bound of each stage
    f = br.fold(p)
    s = br.block_shape(layer, block)[2]
    x64 = maps["x"].astype(np.float64)
    rmid = np.maximum(br.conv3(x64, f["W1"], s) + f["b1"], 0.0)
    Smid = br.conv3(np.abs(x64), np.abs(f["W1"]), s) + np.abs(f["b1"])
    assert br.ratio(maps["mid"], rmid, br.dot_bound(rmid, Smid, f["W1"].shape[1], br.REF_EXTRA)) <= 1.0
    skip = (x64, np.abs(x64)) if f["Wd"] is None else (x64[:, ::s, ::s] @ f["Wd"].astype(np.float64).T,
                                                       np.abs(x64)[:, ::s, ::s] @ np.abs(f["Wd"]).astype(np.float64).T)
    m64 = maps["mid"].astype(np.float64)
    ry = np.maximum(br.conv3(m64, f["W2"], 1) + f["b2"] + skip[0], 0.0)
    Sy = br.conv3(m64, np.abs(f["W2"]), 1) + np.abs(f["b2"]) + skip[1]
    K2 = f["W2"].shape[1] + (0 if f["Wd"] is None else f["Wd"].shape[1])
    assert br.ratio(maps["y"], ry, br.dot_bound(ry, Sy, K2 + 1, 2 * br.REF_EXTRA)) <= 1.0  # two BatchNorms meet in z


@pytest.mark.parametrize("layer,block,shape", FIXTURE)
def test_restatement_against_autograd(layer, block, shape):
    """Folded gradients + unfold against torch's float64 autograd of the unfolded block in eval(), on torch's own mid
    and y (so both sides read the same ReLU masks), element by element within the float32-reference form of the
    bound: that form already holds the one difference between the two functions, the float32 rounding of W' and b'
    (two of its REF_EXTRA roundings per term), and a float64 evaluation rounds less than the float32 one it was
    derived for."""
    _, cout, s, ds = br.block_shape(layer, block)
    p = br.draw_params(layer, block, 7)
    c = br.draw_case(layer, block, *shape, 11)
    leaves, tmid, ty = _torch_block(p, c["x"], s)
    ty.backward(_t(c["gy"].transpose(0, 3, 1, 2)))
    nhwc = lambda t: t.detach().numpy().transpose(0, 2, 3, 1)  # noqa: E731
    maps = dict(x=c["x"], mid=nhwc(tmid), y=nhwc(ty), gy=c["gy"])
    R, E = br.unfolded(layer, block, p, maps, f32=True)
    got = {"dx": nhwc(leaves["x"].grad)}
    for conv, bn, _, _ in br.PAIRS[:3 if ds else 2]:
        got[conv + ".weight"] = leaves[conv].grad.numpy()
        got[bn + ".weight"], got[bn + ".bias"] = leaves[bn + ".g"].grad.numpy(), leaves[bn + ".b"].grad.numpy()
    assert set(got) == set(R)
    q = {k: br.ratio(got[k], R[k], E[k]) for k in got}
    assert max(q.values()) <= 1.0, q
    f = br.fold(p)
    x64 = c["x"].astype(np.float64)
    rmid = np.maximum(br.conv3(x64, f["W1"], s) + f["b1"], 0.0)
    Smid = br.conv3(np.abs(x64), np.abs(f["W1"]), s) + np.abs(f["b1"])
    assert br.ratio(maps["mid"], rmid, br.dot_bound(rmid, Smid, f["W1"].shape[1], br.REF_EXTRA)) <= 1.0


@pytest.mark.parametrize("layer,block,shape", [(1, 1, (1, 3, 4)), (2, 0, (1, 5, 4))])
def test_central_difference(layer, block, shape):
    """L(t) = <gy, y(x + t d)> differentiated at t = 0.  The case is built away from the ReLU kinks: t is half the
    smallest |pre-activation| / max |d pre-activation / dt|, so no pre-activation changes sign on [-t, t] and L is there
    a polynomial of degree 2 in t (two stacked convolutions; x enters the skip linearly), whose central difference has
    no truncation error.  What is left is float64 rounding.  A term of L passes through at most n = K1 + K2 + 8
    roundings (the two dot products, two bias additions, the skip, the product with gy and the final sum's share), so
    each evaluation errs by at most n 2^-53 S_L, S_L = L on absolute values at |x| + t |d|, and the quotient by
    n 2^-53 S_L / t.  <dx, d> adds its own sum over x.size terms of the same chain: (n + x.size) 2^-53 <S_dx, |d|>
    with S_dx the backward on absolute values under the same masks."""
    _, _, s, _ = br.block_shape(layer, block)
    f = br.fold(br.draw_params(layer, block, 3))
    c = br.draw_case(layer, block, *shape, 5)
    x = c["x"].astype(np.float64)
    rng = np.random.default_rng(9)
    d = rng.standard_normal(x.shape)
    gy = c["gy"].astype(np.float64)
    W1, W2 = f["W1"].astype(np.float64), f["W2"].astype(np.float64)
    fabs = {k: (None if v is None else np.abs(v)) for k, v in f.items()}
    skip = (lambda v, g: v) if f["Wd"] is None else (lambda v, g: v[:, ::s, ::s] @ g["Wd"].astype(np.float64).T)
    z1 = br.conv3(x, W1, s) + f["b1"]
    dz1 = br.conv3(np.abs(d), np.abs(W1), s)
    z2 = br.conv3(np.maximum(z1, 0), W2, 1) + f["b2"] + skip(x, f)
    dz2 = br.conv3(dz1, np.abs(W2), 1) + skip(np.abs(d), fabs)
    t = 0.5 * min(np.min(np.abs(z1) / dz1), np.min(np.abs(z2) / dz2))
    assert t > 1e-9
    L = lambda v: float((br.forward(v, f, s)[1] * gy).sum())  # noqa: E731
    mid, y = br.forward(x, f, s)
    R, _ = br.backward(x, mid, y, gy, f, s)
    fd = (L(x + t * d) - L(x - t * d)) / (2 * t)
    exact = float((R["dx"] * d).sum())
    n = W1.shape[1] + W2.shape[1] + (0 if f["Wd"] is None else f["Wd"].shape[1]) + 8
    S_L = float((br.forward(np.abs(x) + t * np.abs(d), fabs, s)[1] * np.abs(gy)).sum())
    S_dx = br.backward(np.abs(x), mid, y, np.abs(gy), fabs, s)[0]["dx"]
    tol = n * br.U53 * S_L / t + (n + x.size) * br.U53 * float((S_dx * np.abs(d)).sum())
    assert abs(fd - exact) <= tol, (fd, exact, t, tol)


@pytest.mark.parametrize("s,h,w", [(1, 4, 5), (2, 5, 7), (2, 4, 6), (2, 1, 1)])
def test_adjoint_identity(s, h, w):
    rng = np.random.default_rng(h * 10 + w)
    x = rng.standard_normal((2, h, w, 3))
    W = rng.standard_normal((4, 27))
    yv = br.conv3(x, W, s)
    g = rng.standard_normal(yv.shape)
    lhs, rhs = float((br.dgrad3(g, W, s, h, w) * x).sum()), float((g * yv).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((np.abs(g) * br.conv3(np.abs(x), np.abs(W), s)).sum())


def test_bn_unfold_against_autograd():
    rng = np.random.default_rng(2)
    w = rng.standard_normal((6, 4, 3, 3)).astype(np.float32)
    bn = (rng.uniform(0.5, 1.5, 6).astype(np.float32), rng.standard_normal(6).astype(np.float32),
          rng.standard_normal(6).astype(np.float32), rng.uniform(0.5, 1.5, 6).astype(np.float32))
    x = _t(rng.standard_normal((2, 4, 5, 5)))
    g = _t(rng.standard_normal((2, 6, 5, 5)))
    tw, tg, tb = (_t(v).requires_grad_(True) for v in (w, bn[0], bn[1]))
    F.batch_norm(F.conv2d(x, tw, padding=1), _t(bn[2]), _t(bn[3]), tg, tb, False, 0.1, br.EPS).backward(g)
    # the folded form's gradients in float64: y = conv(x; W') + b'
    sc = bn[0].astype(np.float64) / np.sqrt(bn[3].astype(np.float64) + br.EPS)
    wf = (_t(w) * _t(sc).view(-1, 1, 1, 1)).detach().requires_grad_(True)
    bf = _t(bn[1].astype(np.float64) - bn[2].astype(np.float64) * sc).requires_grad_(True)
    F.conv2d(x, wf, bf, padding=1).backward(g)
    (dW, dg, dbt), _ = br.bn_unfold(w, bn, wf.grad.numpy(), bf.grad.numpy())
    for got, ref in ((dW, tw.grad), (dg, tg.grad), (dbt, tb.grad)):
        assert np.max(np.abs(got - ref.numpy())) <= 1e-12 * max(1.0, float(ref.abs().max()))


def _one_hot_reach(h, w, iy, ix):
    """Output pixels whose gradient reaches input (iy, ix) at stride 2: dgrad of each one-hot output pixel."""
    oh, ow = -(-h // 2), -(-w // 2)
    W = np.ones((1, 9))
    hit = []
    for oy in range(oh):
        for ox in range(ow):
            g = np.zeros((1, oh, ow, 1))
            g[0, oy, ox, 0] = 1.0
            if br.dgrad3(g, W, 2, h, w)[0, iy, ix, 0] != 0:
                hit.append((oy, ox))
    return hit


def test_stride2_known_answers():
    """An even input row reaches one output row (ky = 1), an odd one two (ky = 0 and 2); the last row and column of an
    odd-sized map reach the bottom and right padding: only the last output pixel sees them, through its centre."""
    h, w = 5, 7
    assert _one_hot_reach(h, w, 2, 2) == [(1, 1)]
    assert _one_hot_reach(h, w, 1, 2) == [(0, 1), (1, 1)]
    assert _one_hot_reach(h, w, 2, 3) == [(1, 1), (1, 2)]
    assert _one_hot_reach(h, w, 1, 1) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert _one_hot_reach(h, w, 4, 6) == [(2, 3)]
    # the tap each one uses: W one-hot at (ky, kx)
    g = np.zeros((1, 3, 4, 1))
    g[0, 1, 1, 0] = 1.0
    for ky in range(3):
        for kx in range(3):
            W = np.zeros((1, 9))
            W[0, ky * 3 + kx] = 1.0
            d = br.dgrad3(g, W, 2, h, w)[0, :, :, 0]
            assert np.argwhere(d != 0).tolist() == [[2 * 1 - 1 + ky, 2 * 1 - 1 + kx]]
    # even sizes: the last input row is odd and reaches only the last output row (no output row below it)
    assert _one_hot_reach(4, 6, 3, 5) == [(1, 2)]
    assert _one_hot_reach(4, 6, 3, 4) == [(1, 2)]
