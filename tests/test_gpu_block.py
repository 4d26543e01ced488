"""sfa_model_block_forward, sfa_model_block_grad and sfa_bn_unfold_grad on the GPU (csrc/block.hip) against the numpy
float64 restatement (tests/block_restatement.py) within the bounds derived there: all seven distinct block shapes at
both strides and odd sizes, several split-K chunk caps, every combination of wanted outputs with guard bands,
the reference fixture, bit-identical runs, graph replay, the forward at the per-stage gate (odd sizes at stride 2
included) and every error return."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import block_restatement as br
import golden_io
from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

_CACHE = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 64  # floats on either side of every output buffer

# (layer, block, (B, h, w)): stride 1 at C = 64, 128, 256, 512, stride 2 at layer2.0, layer3.0, layer4.0
S1 = [(L, 1, s) for L in (1, 2, 3, 4) for s in ((1, 1, 1), (2, 3, 5), (1, 2, 7))] + [(1, 0, (1, 2, 70))]
S2 = [(L, 0, s) for L in (2, 3, 4) for s in ((1, 1, 1), (2, 2, 2), (2, 5, 7), (1, 4, 6))] + [(2, 0, (1, 3, 66))]
CASES = S1 + S2
CAPS = (0, 3, 17)


def _params(layer, block):
    key = ("p", layer, block)
    if key not in _CACHE:
        _CACHE[key] = br.draw_params(layer, block, 100 + 10 * layer + block)
    return _CACHE[key]


def _engine(gpu):
    if "eng" not in _CACHE:
        arch = _lib.make_arch(dict(runtime.DEFAULT_HEADS))
        sd = dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), 11))
        for L in (1, 2, 3, 4):
            for b in (0, 1):
                for k, v in br.state_entries(L, b, _params(L, b)).items():
                    assert sd[k].shape == v.shape, k
                    sd[k] = v.copy()
        _CACHE["eng"] = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    return _CACHE["eng"]


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _case(gpu, layer, block, shape):
    key = ("case", layer, block, shape)
    if key not in _CACHE:
        c = br.draw_case(layer, block, *shape, 1000 * layer + 100 * block + sum(shape))
        c["dev"] = {k: _dev(gpu, c[k]) for k in ("x", "mid", "y", "gy")}
        _CACHE[key] = c
    return _CACHE[key]


def _shapes(layer, block, shape):
    cin, cout, s, ds = br.block_shape(layer, block)
    B, h, w = shape
    return [(B, h, w, cin), (cout, cin, 3, 3), (cout,), (cout, cout, 3, 3), (cout,), (cout, cin, 1, 1)], ds


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
    eng = _engine(gpu)
    c = _case(gpu, layer, block, shape)
    shapes, ds = _shapes(layer, block, shape)
    want = [True] * 5 + [ds] if want is None else list(want)
    g = Guarded(gpu, shapes, want)
    d = c["dev"]
    dx, dp = eng.block_grad(layer, block, d["x"], d["mid"], d["y"], d["gy"], want_x=want[0], want_params=want[1:],
                            out=(g.outs[0], g.outs[1:]), max_chunk_pixels=cap)
    torch.cuda.synchronize()
    assert g.intact(), "a guard band was written"
    return [None if t is None else t.cpu().numpy() for t in [dx] + list(dp)]


def _ratio(got, ref, bound):
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), "an element was not written"
    err, bound = np.abs(got - ref), np.broadcast_to(bound, ref.shape)
    exact = bound == 0  # an all-zero sum: nothing to round
    assert not err[exact].any()
    return float(np.max(err[~exact] / bound[~exact])) if (~exact).any() else 0.0


@pytest.mark.parametrize("case", range(len(CASES)))
def test_gradients_within_the_derived_bounds(gpu, case):
    layer, block, shape = CASES[case]
    eng = _engine(gpu)
    c = _case(gpu, layer, block, shape)
    _, cout, s, ds = br.block_shape(layer, block)
    f = br.fold(_params(layer, block))
    B, h, w = shape
    npix = B * -(-h // s) * -(-w // s)
    for cap in CAPS:
        kcs = [eng.block_grad_chunk_pixels(layer, block, which, B, h, w, cap) for which in (0, 1, 2)]
        want_kc = min(npix, cap if cap else 2048)
        assert kcs[:2] == [want_kc, want_kc] and kcs[2] == (want_kc if ds else 0), (kcs, want_kc)
        R, E = br.backward(c["x"], c["mid"], c["y"], c["gy"], f, s, Kc=want_kc)
        got = _grad(gpu, layer, block, shape, cap=cap)
        q = {k: _ratio(g, R[k], E[k]) for k, g in zip(br.GRADS, got) if g is not None}
        assert set(q) == set(k for k in br.GRADS if R[k] is not None)
        print(f"block grad layer{layer}.{block} {shape} cap {cap}: error / bound " + " ".join(f"{k} {v:.4f}" for k, v in q.items()))
        assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("layer,block,shape", [(1, 1, (2, 3, 5)), (2, 0, (2, 5, 7))])
def test_every_combination_of_wanted_outputs(gpu, layer, block, shape):
    """Each output of each subset equals the full run's bit for bit; the others stay None; guard bands intact."""
    _, ds = _shapes(layer, block, shape)
    full = _grad(gpu, layer, block, shape, cap=17)
    n = 6 if ds else 5
    for want in itertools.product((False, True), repeat=n):
        if not any(want):
            continue
        want = list(want) + [False] * (6 - n)
        got = _grad(gpu, layer, block, shape, want=want, cap=17)
        for k, (g, fl, wnt) in enumerate(zip(got, full, want)):
            assert (g is not None) == wnt
            if wnt:
                assert np.array_equal(g, fl, equal_nan=False), (want, br.GRADS[k])


def test_x_may_be_null_without_a_gradient_that_reads_it(gpu):
    eng = _engine(gpu)
    layer, block, shape = 2, 0, (2, 5, 7)
    d = _case(gpu, layer, block, shape)["dev"]
    full = _grad(gpu, layer, block, shape)
    shapes, _ = _shapes(layer, block, shape)
    B, h, w = shape
    outs = [torch.empty(s, device=gpu) for s in shapes]
    dparams = (ctypes.c_void_p * 5)(None, outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), None)
    need = eng.block_grad_workspace_bytes(layer, block, B, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    rc = _lib.lib().sfa_model_block_grad(eng._h, layer, block, None, d["mid"].data_ptr(), d["y"].data_ptr(),
                                         d["gy"].data_ptr(), B, h, w, outs[0].data_ptr(), dparams, 0, ws.data_ptr(), need,
                                         _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().sfa_last_error_string()
    for k in (0, 2, 3, 4):
        assert np.array_equal(outs[k].cpu().numpy(), full[k])


def test_two_runs_and_a_graph_replay_are_bit_equal(gpu):
    eng = _engine(gpu)
    layer, block, shape = 3, 0, (2, 5, 7)
    B, h, w = shape
    d = _case(gpu, layer, block, shape)["dev"]
    first = _grad(gpu, layer, block, shape, cap=3)
    again = _grad(gpu, layer, block, shape, cap=3)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    shapes, _ = _shapes(layer, block, shape)
    outs = [torch.full(s, float("nan"), device=gpu) for s in shapes]
    ws = torch.empty(eng.block_grad_workspace_bytes(layer, block, B, h, w, 3), dtype=torch.uint8, device=gpu)
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            eng.block_grad(layer, block, d["x"], d["mid"], d["y"], d["gy"], out=(outs[0], outs[1:]), max_chunk_pixels=3,
                           workspace=ws)
    for t in outs:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, t in zip(first, outs):
        assert np.array_equal(a, t.cpu().numpy())


FWD = [(1, 0, (2, 3, 5)), (1, 1, (1, 2, 70)), (2, 0, (2, 4, 6)), (2, 1, (2, 3, 5)), (3, 0, (1, 6, 4)), (3, 1, (1, 3, 2)),
       (4, 0, (2, 2, 2)), (4, 1, (1, 1, 1)), (2, 0, (1, 2, 66)),
       # odd sizes at stride 2: the last output row and column read the bottom and right padding
       (2, 0, (2, 5, 7)), (2, 0, (1, 1, 1)), (2, 0, (1, 3, 66)), (3, 0, (2, 5, 7)), (3, 0, (1, 4, 7)), (4, 0, (2, 5, 7)),
       (4, 0, (1, 3, 3))]


@pytest.mark.parametrize("layer,block,shape", FWD)
def test_forward_at_the_stage_gate(gpu, layer, block, shape):
    """mid from x, and y from the device's own mid, each within 1e-5 max(1, |v|) of the restatement."""
    eng = _engine(gpu)
    _, _, s, _ = br.block_shape(layer, block)
    f = br.fold(_params(layer, block))
    c = _case(gpu, layer, block, shape)
    mid, y = eng.block_forward(layer, block, c["dev"]["x"])
    torch.cuda.synchronize()
    mid, y = mid.cpu().numpy(), y.cpu().numpy()
    rmid, _ = br.forward(c["x"], f, s)
    x64 = c["x"].astype(np.float64)
    skip = x64 if f["Wd"] is None else x64[:, ::s, ::s] @ f["Wd"].astype(np.float64).T
    ry = np.maximum(br.conv3(mid, f["W2"], 1) + f["b2"].astype(np.float64) + skip, 0.0)
    q = [float(np.max(np.abs(g - r) / np.maximum(1.0, np.abs(r)))) for g, r in ((mid, rmid), (y, ry))]
    print(f"block forward layer{layer}.{block} {shape}: mid {q[0]:.3e} y {q[1]:.3e}")
    assert max(q) <= 1e-5, q


def _golden_engine(gpu, g):
    if "geng" not in _CACHE:
        arch = _lib.make_arch(dict(runtime.DEFAULT_HEADS))
        sd = dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), 11))
        ps = {}
        for c in g["cases"]:
            L, b = int(g[f"{c}/layer"]), int(g[f"{c}/block"])
            ps[(L, b)] = br.draw_params(L, b, int(g[f"{c}/param_seed"]))
            for k, v in br.state_entries(L, b, ps[(L, b)]).items():
                sd[k] = v.copy()
        _CACHE["geng"] = (runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu), ps)
    return _CACHE["geng"]


@pytest.mark.parametrize("name", ["L1b0_B2_3x5", "L2b0_B2_5x7", "L2b0_B1_4x6"])
def test_reference_fixture(gpu, name):
    """The reference's BasicBlock (tests/golden/block_golden*.npz) on its own stored maps: sfa_model_block_grad then
    sfa_bn_unfold_grad within the device's bound of the restatement, the reference within its float32 bound of it,
    so the two within the sum of the bounds of each other, element by element."""
    if "golden" not in _CACHE:
        _CACHE["golden"] = golden_io.load(GOLDEN, "block_golden")
    g = _CACHE["golden"]
    assert name in list(g["cases"])
    eng, ps = _golden_engine(gpu, g)
    layer, block = int(g[f"{name}/layer"]), int(g[f"{name}/block"])
    p = ps[(layer, block)]
    maps = {k: g[f"{name}/{k}"] for k in ("x", "mid", "y", "gy")}
    B, h, w, _ = maps["x"].shape
    d = {k: _dev(gpu, v) for k, v in maps.items()}
    dx, dp = eng.block_grad(layer, block, d["x"], d["mid"], d["y"], d["gy"], max_chunk_pixels=17)
    got = {"dx": dx}
    for i, (conv, bn, _, _) in enumerate(br.PAIRS):
        if conv not in p:
            continue
        gam, _, mu, var = p[bn]
        got[conv + ".weight"], got[bn + ".weight"], got[bn + ".bias"] = runtime.bn_unfold_grad(
            _dev(gpu, p[conv]), _dev(gpu, gam), _dev(gpu, mu), _dev(gpu, var), br.EPS, dp[(0, 2, 4)[i]], dp[(1, 3, 3)[i]])
    torch.cuda.synchronize()
    kc = eng.block_grad_chunk_pixels(layer, block, 0, B, h, w, 17)
    R, E = br.unfolded(layer, block, p, maps, Kc=kc)
    _, Eref = br.unfolded(layer, block, p, maps, f32=True)
    assert set(got) == set(R)
    q = {}
    for k, t in got.items():
        dev = t.cpu().numpy().astype(np.float64).reshape(R[k].shape)
        q[k] = (br.ratio(dev, R[k], E[k]), br.ratio(g[f"{name}/{k}"], R[k], Eref[k]),
                br.ratio(dev, g[f"{name}/{k}"].astype(np.float64).reshape(R[k].shape), E[k] + Eref[k]))
    print(f"block fixture {name}: (device, reference, device - reference) / bound " +
          " ".join(f"{k} {a:.4f} {b:.4f} {c:.4f}" for k, (a, b, c) in q.items()))
    assert max(max(v) for v in q.values()) <= 1.0, q


def test_bn_unfold_within_the_derived_bounds(gpu):
    rng = np.random.default_rng(4)
    for cout, cin, k in ((64, 64, 3), (128, 64, 1), (512, 512, 3)):
        w = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(k * k * cin)).astype(np.float32)
        bn = (rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32),
              (0.3 * rng.standard_normal(cout)).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32))
        dWf = rng.standard_normal(w.shape).astype(np.float32)
        dbf = rng.standard_normal(cout).astype(np.float32)
        got = runtime.bn_unfold_grad(_dev(gpu, w), _dev(gpu, bn[0]), _dev(gpu, bn[2]), _dev(gpu, bn[3]), br.EPS,
                                     _dev(gpu, dWf), _dev(gpu, dbf))
        torch.cuda.synchronize()
        R, E = br.bn_unfold(w, bn, dWf, dbf)
        assert _ratio(got[0].cpu().numpy(), R[0], E[0]) <= 1.0
        assert _ratio(got[1].cpu().numpy(), R[1], E[1]) <= 1.0
        assert np.array_equal(got[2].cpu().numpy(), dbf)
        only = runtime.bn_unfold_grad(_dev(gpu, w), _dev(gpu, bn[0]), _dev(gpu, bn[2]), _dev(gpu, bn[3]), br.EPS,
                                      _dev(gpu, dWf), _dev(gpu, dbf), want=(True, False, False))
        assert only[1] is None and only[2] is None and torch.equal(only[0], got[0])


def test_refusals(gpu):
    L = _lib.lib()
    eng = _engine(gpu)
    layer, block, (B, h, w) = 2, 0, (2, 5, 7)
    d = _case(gpu, layer, block, (B, h, w))["dev"]
    shapes, _ = _shapes(layer, block, (B, h, w))
    outs = [torch.empty(s, device=gpu) for s in shapes]
    need = eng.block_grad_workspace_bytes(layer, block, B, h, w)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=gpu)
    sp = _lib.stream_ptr(gpu)

    def grad(layer=layer, block=block, x=d["x"].data_ptr(), mid=d["mid"].data_ptr(), y=d["y"].data_ptr(),
             gy=d["gy"].data_ptr(), B=B, h=h, w=w, gx=outs[0].data_ptr(), dp="all", cap=0, wsp=ws.data_ptr(), nb=need, m=eng._h):
        if dp == "all":
            dp = [t.data_ptr() for t in outs[1:]]
        arr = None if dp is None else (ctypes.c_void_p * 5)(*dp)
        return L.sfa_model_block_grad(m, layer, block, x, mid, y, gy, B, h, w, gx, arr, cap, wsp, nb, sp)

    inv = -1  # SFA_E_INVALID
    assert grad() == 0
    for kw in (dict(m=None), dict(mid=None), dict(y=None), dict(gy=None), dict(wsp=None), dict(x=None),
               dict(layer=0), dict(layer=5), dict(block=-1), dict(block=2), dict(B=0), dict(h=0), dict(w=-1),
               dict(cap=-1), dict(nb=need - 1), dict(gx=None, dp=None), dict(gx=outs[0].data_ptr() + 4),
               dict(wsp=ws.data_ptr() + 4), dict(gy=d["gy"].data_ptr() + 8), dict(B=1 << 20, h=64, w=64)):
        assert grad(**kw) == inv, kw
    # a dWd' pointer on a block without a downsample
    d1 = _case(gpu, 2, 1, (2, 3, 5))["dev"]
    sh1, _ = _shapes(2, 1, (2, 3, 5))
    o1 = [torch.empty(s, device=gpu) for s in sh1]
    big = torch.empty(eng.block_grad_workspace_bytes(2, 1, 2, 3, 5), dtype=torch.uint8, device=gpu)
    arr = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in o1[1:]])
    assert L.sfa_model_block_grad(eng._h, 2, 1, d1["x"].data_ptr(), d1["mid"].data_ptr(), d1["y"].data_ptr(),
                                  d1["gy"].data_ptr(), 2, 3, 5, o1[0].data_ptr(), arr, 0, big.data_ptr(), big.numel(), sp) == inv
    assert eng.block_grad_workspace_bytes(2, 0, 2, 5, 7, -1) == 0
    assert eng.block_grad_workspace_bytes(5, 0, 2, 5, 7) == 0
    assert eng.block_grad_chunk_pixels(2, 1, 2, 2, 3, 5) == 0  # no dWd' there
    # forward: the same argument checks
    fneed = eng.block_forward_workspace_bytes(2, 0, 2, 4, 6)
    fws = torch.empty(fneed, dtype=torch.uint8, device=gpu)
    x = torch.zeros((2, 4, 6, 64), device=gpu)
    mo, yo = torch.empty((2, 2, 3, 128), device=gpu), torch.empty((2, 2, 3, 128), device=gpu)
    fwd = lambda layer=2, x=x.data_ptr(), h=4, w=6, nb=fneed, m=eng._h, wsp=fws.data_ptr(): L.sfa_model_block_forward(  # noqa: E731
        m, layer, 0, x, 2, h, w, mo.data_ptr(), yo.data_ptr(), wsp, nb, sp)
    assert fwd() == 0
    for kw in (dict(m=None), dict(x=None), dict(layer=0), dict(h=0), dict(nb=fneed - 1), dict(wsp=None),
               dict(x=x.data_ptr() + 4)):
        assert fwd(**kw) == inv, kw
    torch.cuda.synchronize()
    # bn unfold
    t = torch.zeros(64, device=gpu)
    W = torch.zeros((64, 9), device=gpu)
    unf = lambda W=W.data_ptr(), g=t.data_ptr(), dWf=W.data_ptr(), dbf=t.data_ptr(), C=64, K=9, eps=1e-5, dW=W.data_ptr(), dg=t.data_ptr(): \
        L.sfa_bn_unfold_grad(W, g, t.data_ptr(), t.data_ptr(), eps, dWf, dbf, C, K, dW, dg, None, sp)  # noqa: E731
    for kw in (dict(C=0), dict(K=0), dict(eps=-1.0), dict(g=None), dict(dWf=None), dict(dbf=None), dict(W=None),
               dict(dW=None, dg=None)):
        assert unf(**kw) == inv, kw


def test_deconv_model_is_unsupported(gpu):
    arch = _lib.make_arch(dict(runtime.DEFAULT_HEADS), backbone=_lib.BACKBONE_DECONV)
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 3)
    eng = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    t = torch.zeros((1, 2, 2, 64), device=gpu)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    sp = _lib.stream_ptr(gpu)
    L = _lib.lib()
    assert L.sfa_model_block_forward(eng._h, 1, 0, t.data_ptr(), 1, 2, 2, t.data_ptr(), t.data_ptr(), ws.data_ptr(),
                                     ws.numel(), sp) == -2
    assert L.sfa_model_block_grad(eng._h, 1, 0, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 2, 2,
                                  t.data_ptr(), None, 0, ws.data_ptr(), ws.numel(), sp) == -2
    with pytest.raises(ValueError):
        eng.block_forward(1, 0, t)
