"""sfa_block_train_forward and sfa_block_train_grad on the GPU (csrc/block_train.hip) against the numpy float64
restatement (tests/block_train_restatement.py) within the bounds derived there: every stage of the forward from the
device's own inputs, every gradient from the device's own maps and statistics, at split-K / statistics caps 0, 3 and
17; every combination of wanted outputs with guard bands; bit-identical runs and a graph replay of forward +
gradient; the reference fixture (tests/golden/block_train_golden*.npz) with its running buffers; every refusal with
sentinel-filled outputs untouched."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import block_train_restatement as tr
import golden_io
from sfa_hip import _lib, runtime

pytestmark = pytest.mark.gpu

_CACHE = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 64

# stride 1 at C = 64, 128, 256, 512: n = 2 (the fewest allowed), odd sizes, a map that crosses a 64-pixel tile
S1 = [(L, 1, s) for L in (1, 2, 3, 4) for s in ((2, 1, 1), (2, 3, 5), (1, 2, 70))]
# stride 2 with a downsample: odd sizes whose last taps read the padding
S2 = [(L, 0, s) for L in (2, 3, 4) for s in ((2, 2, 2), (2, 5, 7), (1, 4, 6))] + [(2, 0, (1, 3, 66))]
CASES = S1 + S2
CAPS = (0, 3, 17)


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _params(gpu, layer, block):
    key = ("p", layer, block)
    if key not in _CACHE:
        p = tr.draw_params(layer, block, 500 + 10 * layer + block)
        _CACHE[key] = (p, [_dev(gpu, a) for a in tr.param_list(p)])
    return _CACHE[key]


def _case(gpu, layer, block, shape):
    key = ("case", layer, block, shape)
    if key not in _CACHE:
        x, gy = tr.draw_x(layer, block, *shape, 2000 * layer + 100 * block + sum(shape))
        _CACHE[key] = dict(x=x, gy=gy, dx=_dev(gpu, x), dgy=_dev(gpu, gy))
    return _CACHE[key]


def _forward(gpu, layer, block, shape, cap=0):
    key = ("fwd", layer, block, shape, cap)
    if key not in _CACHE:
        c = _case(gpu, layer, block, shape)
        m = runtime.block_train_forward(layer, block, c["dx"], _params(gpu, layer, block)[1], tr.EPS, max_chunk_pixels=cap)
        torch.cuda.synchronize()
        _CACHE[key] = (m, {k: (None if v is None else v.cpu().numpy()) for k, v in m.items()})
    return _CACHE[key]


def _out_shapes(layer, block, shape):
    cin, cout, _, ds = tr.block_shape(layer, block)
    B, h, w = shape
    sh = [(B, h, w, cin), (cout, cin, 3, 3), (cout,), (cout,), (cout, cout, 3, 3), (cout,), (cout,)]
    return sh + ([(cout, cin, 1, 1), (cout,), (cout,)] if ds else []), ds


class Guarded:
    """Output buffers cut from sentinel-filled storage with GUARD floats on either side."""

    def __init__(self, gpu, shapes, want):
        self.bufs, self.outs = [], []
        for s, wnt in zip(shapes, want):
            if not wnt:
                self.bufs.append(None)
                self.outs.append(None)
                continue
            n = int(np.prod(s))
            buf = torch.full((n + 2 * GUARD,), -7.25, device=gpu)
            buf[GUARD:GUARD + n] = float("nan")
            self.bufs.append(buf)
            self.outs.append(buf[GUARD:GUARD + n].view(s))

    def intact(self):
        return all(b is None or (bool((b[:GUARD] == -7.25).all()) and bool((b[-GUARD:] == -7.25).all())) for b in self.bufs)


def _grad(gpu, layer, block, shape, want=None, cap=0):
    c = _case(gpu, layer, block, shape)
    m, _ = _forward(gpu, layer, block, shape)
    shapes, ds = _out_shapes(layer, block, shape)
    want = [True] * len(shapes) if want is None else list(want)
    g = Guarded(gpu, shapes, want)
    wp = want[1:] + [False] * (10 - len(want))
    outs = g.outs[1:] + [None] * (10 - len(want))
    dx, dp = runtime.block_train_grad(layer, block, c["dx"], m, c["dgy"], _params(gpu, layer, block)[1], tr.EPS,
                                      want_x=want[0], want_params=wp, out=(g.outs[0], outs), max_chunk_pixels=cap)
    torch.cuda.synchronize()
    assert g.intact(), "a guard band was written"
    return [None if t is None else t.cpu().numpy() for t in ([dx] + list(dp))[:len(shapes)]]


def _ratio(got, ref, bound):
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    assert np.isfinite(got).all(), "an element was not written"
    err, bound = np.abs(got - ref), np.broadcast_to(bound, np.shape(ref))
    exact = bound == 0
    assert not err[exact].any()
    return float(np.max(err[~exact] / bound[~exact])) if (~exact).any() else 0.0


def _forward_ratios(x, p, s, m, eps=tr.EPS):
    """error / bound of every stage of the forward, each stage from the device's own inputs."""
    q = {}
    st = m["stats"]
    bns = [("z1", "conv1", "bn1", x, s), ("z2", "conv2", "bn2", m["mid"], 1)]
    if "convd" in p:
        bns.append(("zd", "convd", "bnd", x, s))
    cf = []
    for i, (zk, ck, bk, src, stride) in enumerate(bns):
        r, e = tr.conv_stage(src, p[ck], stride)
        q[zk] = _ratio(m[zk], r, e)
        (mean, var), (Em, Ev) = tr.stats_stage(m[zk])
        q[bk + ".mean"], q[bk + ".var"] = _ratio(st[i, 0], mean, Em), _ratio(st[i, 1], var, Ev)
        cf.append(tr.coef(p[bk][0], p[bk][1], st[i, 0], st[i, 1], eps))
    r, e, _ = tr.apply_stage(m["z1"], cf[0])
    q["mid"] = _ratio(m["mid"], r, e)
    if "convd" in p:
        r, e, _ = tr.apply_stage(m["z2"], cf[1], zd=m["zd"], cd=cf[2])
    else:
        r, e, _ = tr.apply_stage(m["z2"], cf[1], x=x)
    q["y"] = _ratio(m["y"], r, e)
    return q


@pytest.mark.parametrize("case", range(len(CASES)))
def test_forward_and_gradients_within_the_derived_bounds(gpu, case):
    layer, block, shape = CASES[case]
    _, _, s, ds = tr.block_shape(layer, block)
    p = _params(gpu, layer, block)[0]
    c = _case(gpu, layer, block, shape)
    B, h, w = shape
    npix = B * -(-h // s) * -(-w // s)
    keys = ["dx"] + list(tr.PARAMS[:9 if ds else 6])
    for cap in CAPS:
        _, m = _forward(gpu, layer, block, shape, cap)
        qf = _forward_ratios(c["x"], p, s, m)
        print(f"block train forward layer{layer}.{block} {shape} cap {cap}: error / bound " + " ".join(f"{k} {v:.4f}" for k, v in qf.items()))
        assert max(qf.values()) <= 1.0, qf
        _, m0 = _forward(gpu, layer, block, shape)
        kcs = [runtime.block_train_chunk_pixels(layer, block, which, B, h, w, cap) for which in (0, 1, 2, 3)]
        want_kc = min(npix, cap if cap else 2048)
        assert kcs[:2] == [want_kc, want_kc] and kcs[2] == (want_kc if ds else 0), (kcs, want_kc)
        assert kcs[3] == (min(cap, 64) if cap else 64)
        R, E = tr.backward(c["x"], m0, c["gy"], p, s, Kc=want_kc)
        got = _grad(gpu, layer, block, shape, cap=cap)
        q = {k: _ratio(g, R[k], E[k]) for k, g in zip(keys, got)}
        print(f"block train grad layer{layer}.{block} {shape} cap {cap}: error / bound " + " ".join(f"{k} {v:.4f}" for k, v in q.items()))
        assert max(q.values()) <= 1.0, q


def test_statistics_are_the_batchs_not_the_running_ones(gpu):
    layer, block, shape = 2, 0, (2, 5, 7)
    p = _params(gpu, layer, block)[0]
    _, m = _forward(gpu, layer, block, shape)
    for i, bn in enumerate(tr.BNS):
        assert float(np.min(np.abs(m["stats"][i, 0] - p[bn][2]))) > 1.0 and float(np.min(np.abs(m["stats"][i, 1] - p[bn][3]))) > 1.0


@pytest.mark.parametrize("layer,block,shape", [(1, 1, (2, 3, 5)), (2, 0, (2, 5, 7))])
def test_every_combination_of_wanted_outputs(gpu, layer, block, shape):
    """Each output of each subset equals the full run's bit for bit; the others stay None; guard bands intact."""
    shapes, _ = _out_shapes(layer, block, shape)
    full = _grad(gpu, layer, block, shape, cap=17)
    n = len(shapes)
    for want in itertools.product((False, True), repeat=n):
        if not any(want):
            continue
        got = _grad(gpu, layer, block, shape, want=want, cap=17)
        for k, (g, fl, wnt) in enumerate(zip(got, full, want)):
            assert (g is not None) == wnt
            if wnt:
                assert np.array_equal(g, fl, equal_nan=False), (want, k)


def test_forward_outputs_are_written_inside_their_buffers(gpu):
    layer, block, shape = 2, 0, (2, 5, 7)
    cin, cout, s, _ = tr.block_shape(layer, block)
    c = _case(gpu, layer, block, shape)
    osh = (2, 3, 4, cout)
    names = ["z1", "mid", "z2", "zd", "y", "stats"]
    g = Guarded(gpu, [osh] * 5 + [(3, 2, cout)], [True] * 6)
    runtime.block_train_forward(layer, block, c["dx"], _params(gpu, layer, block)[1], tr.EPS, out=dict(zip(names, g.outs)),
                                max_chunk_pixels=3)
    torch.cuda.synchronize()
    assert g.intact()
    _, m = _forward(gpu, layer, block, shape, 3)
    for k, t in zip(names, g.outs):
        assert np.array_equal(t.cpu().numpy(), m[k])


def test_two_runs_and_a_graph_replay_are_bit_equal(gpu):
    layer, block, shape = 3, 0, (2, 5, 7)
    B, h, w = shape
    cin, cout, s, _ = tr.block_shape(layer, block)
    c = _case(gpu, layer, block, shape)
    ps = _params(gpu, layer, block)[1]
    _, m1 = _forward(gpu, layer, block, shape, 3)
    m2 = runtime.block_train_forward(layer, block, c["dx"], ps, tr.EPS, max_chunk_pixels=3)
    for k, v in m2.items():
        assert np.array_equal(v.cpu().numpy(), m1[k]), k
    first = _grad(gpu, layer, block, shape, cap=3)
    again = _grad(gpu, layer, block, shape, cap=3)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    m0, _ = _forward(gpu, layer, block, shape)
    osh = (B, 3, 4, cout)
    names = ["z1", "mid", "z2", "zd", "y", "stats"]
    fo = {k: torch.full(osh if k != "stats" else (3, 2, cout), float("nan"), device=gpu) for k in names}
    shapes, _ = _out_shapes(layer, block, shape)
    go = [torch.full(sh, float("nan"), device=gpu) for sh in shapes]
    fws = torch.empty(runtime.block_train_forward_workspace_bytes(layer, block, B, h, w, 3), dtype=torch.uint8, device=gpu)
    gws = torch.empty(runtime.block_train_grad_workspace_bytes(layer, block, B, h, w, 3), dtype=torch.uint8, device=gpu)
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            runtime.block_train_forward(layer, block, c["dx"], ps, tr.EPS, out=fo, max_chunk_pixels=3, workspace=fws)
            runtime.block_train_grad(layer, block, c["dx"], fo, c["dgy"], ps, tr.EPS, out=(go[0], go[1:]), max_chunk_pixels=3,
                                     workspace=gws)
    for t in list(fo.values()) + go:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k in names:
        assert np.array_equal(fo[k].cpu().numpy(), m1[k]), k
    # the gradient of the replay read the cap-3 forward's maps: the same bits as the eager gradient on them
    dx, dp = runtime.block_train_grad(layer, block, c["dx"], fo, c["dgy"], ps, tr.EPS, max_chunk_pixels=3)
    torch.cuda.synchronize()
    for a, t in zip([dx] + list(dp), go):
        assert np.array_equal(a.cpu().numpy(), t.cpu().numpy())


@pytest.mark.parametrize("name", ["L1b0_B2_3x5", "L2b0_B2_5x7", "L2b0_B1_4x6"])
def test_reference_fixture(gpu, name):
    """The reference's BasicBlock in train() (tests/golden/block_train_golden*.npz).  Gradients: the device on the
    reference's stored maps and statistics within its bound of the restatement, the reference within its float32
    bound, so the two within the sum.  Forward: the device on the stored x against the reference's y, and the
    running buffers after the step, within the sum of both carried bounds."""
    if "golden" not in _CACHE:
        _CACHE["golden"] = golden_io.load(GOLDEN, "block_train_golden")
    g = _CACHE["golden"]
    assert name in list(g["cases"])
    layer, block = int(g[f"{name}/layer"]), int(g[f"{name}/block"])
    _, _, s, ds = tr.block_shape(layer, block)
    p = tr.fixture_params(g, layer, block)
    ps = [_dev(gpu, a) for a in tr.param_list(p)]
    x, gy = g[f"{name}/x"], g[f"{name}/gy"]
    B, h, w, _ = x.shape
    maps = {k: g[f"{name}/{k}"] for k in ["z1", "mid", "z2", "y", "stats"] + (["zd"] if ds else [])}
    dm = {k: _dev(gpu, v) for k, v in maps.items()}
    dm.setdefault("zd", None)
    dx, dp = runtime.block_train_grad(layer, block, _dev(gpu, x), dm, _dev(gpu, gy), ps, tr.EPS, max_chunk_pixels=17)
    m = runtime.block_train_forward(layer, block, _dev(gpu, x), ps, tr.EPS, max_chunk_pixels=17)
    torch.cuda.synchronize()
    keys = ["dx"] + list(tr.PARAMS[:9 if ds else 6])
    kc = runtime.block_train_chunk_pixels(layer, block, 0, B, h, w, 17)
    R, E = tr.backward(x, maps, gy, p, s, Kc=kc)
    _, Eref = tr.backward(x, maps, gy, p, s, f32=True)
    q = {}
    for k, t in zip(keys, [dx] + list(dp)):
        dev = t.cpu().numpy().astype(np.float64).reshape(R[k].shape)
        ref = g[f"{name}/{k}"].astype(np.float64).reshape(R[k].shape)
        q[k] = (tr.ratio(dev, R[k], E[k]), tr.ratio(ref, R[k], Eref[k]), tr.ratio(dev, ref, E[k] + Eref[k]))
    print(f"block train fixture {name}: (device, reference, device - reference) / bound " +
          " ".join(f"{k} {a:.4f} {b:.4f} {c:.4f}" for k, (a, b, c) in q.items()))
    assert max(max(v) for v in q.values()) <= 1.0, q
    # forward: y and the running buffers, the device's own step against the reference's
    V, Ed = tr.forward_chain(x, p, s)
    _, E32 = tr.forward_chain(x, p, s, f32=True)
    qy = tr.ratio(m["y"].cpu().numpy(), g[f"{name}/y"].astype(np.float64), Ed["y"] + E32["y"])
    stats = m["stats"].cpu().numpy().astype(np.float64)
    n = B * maps["y"].shape[1] * maps["y"].shape[2]
    before, after = g[f"{name}/running_before"], g[f"{name}/running_after"]
    qr = []
    for i in range(stats.shape[0]):
        for which in (0, 1):
            buf = torch.from_numpy(before[i, which].copy())
            f = n / (n - 1.0) if which else 1.0
            buf.mul_(1.0 - tr.MOMENTUM).add_(torch.from_numpy(stats[i, which].astype(np.float32)), alpha=tr.MOMENTUM * f)
            bound = tr.running_bound(before[i, which], V["stats"][i, which], Ed["stats"][i, which], n, which) + \
                tr.running_bound(before[i, which], V["stats"][i, which], E32["stats"][i, which], n, which)
            qr.append(tr.ratio(buf.numpy(), after[i, which].astype(np.float64), bound))
            assert float(np.max(np.abs(after[i, which] - before[i, which]))) > 0.05  # the buffers moved
    print(f"block train fixture {name}: y {qy:.4f} running buffers {max(qr):.4f} (device - reference) / bound")
    assert qy <= 1.0 and max(qr) <= 1.0, (qy, qr)


def test_refusals(gpu):
    L = _lib.lib()
    layer, block, (B, h, w) = 2, 0, (2, 5, 7)
    c = _case(gpu, layer, block, (B, h, w))
    m, _ = _forward(gpu, layer, block, (B, h, w))
    ps = _params(gpu, layer, block)[1]
    shapes, _ = _out_shapes(layer, block, (B, h, w))
    SENT = -3.5
    outs = [torch.full(sh, SENT, device=gpu) for sh in shapes]
    fouts = {k: torch.full(tuple(m[k].shape), SENT, device=gpu) for k in m}
    need = runtime.block_train_grad_workspace_bytes(layer, block, B, h, w)
    fneed = runtime.block_train_forward_workspace_bytes(layer, block, B, h, w)
    ws = torch.empty(max(need, fneed) + 16, dtype=torch.uint8, device=gpu)
    sp = _lib.stream_ptr(gpu)
    P = lambda ts: (ctypes.c_void_p * 9)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    inv = -1  # SFA_E_INVALID

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in outs + list(fouts.values()))

    def grad(layer=layer, block=block, x=c["dx"].data_ptr(), z1=m["z1"].data_ptr(), mid=m["mid"].data_ptr(),
             z2=m["z2"].data_ptr(), zd=m["zd"].data_ptr(), y=m["y"].data_ptr(), gy=c["dgy"].data_ptr(),
             st=m["stats"].data_ptr(), par=P(ps), eps=tr.EPS, B=B, h=h, w=w, gx=outs[0].data_ptr(), dp="all", cap=0,
             wsp=ws.data_ptr(), nb=need):
        if dp == "all":
            dp = P(outs[1:])
        return L.sfa_block_train_grad(layer, block, x, z1, mid, z2, zd, y, gy, st, par, eps, B, h, w, gx, dp, cap, wsp, nb, sp)

    def fwd(layer=layer, block=block, x=c["dx"].data_ptr(), par=P(ps), eps=tr.EPS, B=B, h=h, w=w, z1=fouts["z1"].data_ptr(),
            zd=fouts["zd"].data_ptr(), st=fouts["stats"].data_ptr(), cap=0, wsp=ws.data_ptr(), nb=fneed):
        return L.sfa_block_train_forward(layer, block, x, par, eps, B, h, w, z1, fouts["mid"].data_ptr(),
                                         fouts["z2"].data_ptr(), zd, fouts["y"].data_ptr(), st, cap, wsp, nb, sp)

    nogamma = list(ps)
    nogamma[4] = None
    for kw in (dict(x=None), dict(z1=None), dict(mid=None), dict(z2=None), dict(zd=None), dict(y=None), dict(gy=None),
               dict(st=None), dict(par=None), dict(par=P(nogamma)), dict(wsp=None), dict(layer=0), dict(layer=5),
               dict(block=-1), dict(block=2), dict(B=0), dict(h=0), dict(w=-1), dict(cap=-1), dict(eps=-1e-5),
               dict(nb=need - 1), dict(gx=None, dp=None), dict(gx=outs[0].data_ptr() + 4), dict(wsp=ws.data_ptr() + 4),
               dict(gy=c["dgy"].data_ptr() + 8), dict(B=1 << 20, h=64, w=64),
               dict(B=1, h=2, w=2)):  # n = B oh ow = 1: torch's "Expected more than 1 value per channel when training"
        assert grad(**kw) == inv, kw
    nobeta = list(ps)
    nobeta[3] = None
    for kw in (dict(x=None), dict(par=None), dict(par=P(nobeta)), dict(z1=None), dict(zd=None), dict(st=None), dict(wsp=None),
               dict(layer=0), dict(block=2), dict(B=0), dict(h=-1), dict(cap=-1), dict(eps=-1.0), dict(nb=fneed - 1),
               dict(x=c["dx"].data_ptr() + 4), dict(wsp=ws.data_ptr() + 8), dict(B=1 << 20, h=64, w=64), dict(B=1, h=2, w=2),
               dict(B=1, h=1, w=1)):
        assert fwd(**kw) == inv, kw
    assert untouched()
    # a block without a downsample refuses the downsample's pointers; n = 1 at stride 1
    c1 = _case(gpu, 1, 1, (2, 3, 5))
    m1, _ = _forward(gpu, 1, 1, (2, 3, 5))
    p1 = _params(gpu, 1, 1)[1]
    big = torch.empty(runtime.block_train_grad_workspace_bytes(1, 1, 2, 3, 5), dtype=torch.uint8, device=gpu)
    o1 = [torch.full(sh, SENT, device=gpu) for sh in _out_shapes(1, 1, (2, 3, 5))[0]]
    extra = torch.full((64,), SENT, device=gpu)

    def grad1(zd=None, dp=None, B=2):
        return L.sfa_block_train_grad(1, 1, c1["dx"].data_ptr(), m1["z1"].data_ptr(), m1["mid"].data_ptr(), m1["z2"].data_ptr(),
                                      zd, m1["y"].data_ptr(), c1["dgy"].data_ptr(), m1["stats"].data_ptr(), P(p1), tr.EPS, B, 3, 5,
                                      o1[0].data_ptr(), dp, 0, big.data_ptr(), big.numel(), sp)

    assert grad1(dp=P(o1[1:] + [None, extra, None])) == inv
    assert grad1(zd=m1["z1"].data_ptr(), dp=P(o1[1:])) == inv
    assert L.sfa_block_train_grad(1, 1, c1["dx"].data_ptr(), m1["z1"].data_ptr(), m1["mid"].data_ptr(), m1["z2"].data_ptr(), None,
                                  m1["y"].data_ptr(), c1["dgy"].data_ptr(), m1["stats"].data_ptr(), P(p1), tr.EPS, 1, 1, 1,
                                  o1[0].data_ptr(), P(o1[1:]), 0, big.data_ptr(), big.numel(), sp) == inv
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in o1 + [extra])
    assert grad1(dp=P(o1[1:])) == 0 and grad() == 0 and fwd() == 0
    torch.cuda.synchronize()
    for which in (runtime.block_train_forward_workspace_bytes, runtime.block_train_grad_workspace_bytes):
        assert which(1, 1, 1, 1, 1) == 0 and which(2, 0, 1, 2, 2) == 0 and which(5, 0, 2, 5, 7) == 0 and which(2, 0, 2, 5, 7, -1) == 0
        assert which(1, 1, 2, 1, 1) > 0
    assert runtime.block_train_chunk_pixels(2, 1, 2, 2, 3, 5) == 0  # no dWd there
    assert runtime.block_train_chunk_pixels(1, 1, 0, 1, 1, 1) == 0  # n = 1
    with pytest.raises(ValueError):
        runtime.block_train_forward(1, 1, torch.zeros((1, 1, 1, 64), device=gpu), p1)
