"""sfa_stem_train_forward and sfa_stem_train_grad on the GPU (csrc/stem_train.hip) against the numpy float64
restatement (tests/stem_train_restatement.py) within the bounds derived there: every stage of the forward from the
device's own inputs (a and pooled also bit for bit), every gradient from the device's own maps and statistics, at
split-K / statistics caps 0, 3 and 17; every subset of wanted outputs with guard bands; bit-identical runs and a graph
replay of forward + gradient; the reference fixture (tests/golden/stem_train_golden.npz); every refusal with
sentinel-filled outputs untouched."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import golden_io
import stem_train_restatement as st
from sfa_hip import _lib, runtime

pytestmark = pytest.mark.gpu

_CACHE = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 64
# n = 4 and one pooled pixel; an odd 3 x 5 conv map whose last window reads padding; two frames; 468 conv pixels (no
# multiple of the 64-pixel tile); several statistics blocks and K_c = 2048
SHAPES = [(1, 3, 3), (1, 6, 10), (2, 12, 20), (1, 36, 52), (2, 64, 96)]
CAPS = (0, 3, 17)
OUT_SHAPES = lambda B, H, W: [(B, 3, H, W), (64, 3, 7, 7), (64,), (64,)]  # noqa: E731
INVALID, UNSUPPORTED = -1, -2  # SFA_E_INVALID, SFA_E_UNSUPPORTED (include/sfa_hip.h)
FIXTURE = {"b2_12x20": (2, 12, 20), "b1_6x10": (1, 6, 10)}


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _plist(p):
    return [p["conv1"], p["bn1"][0], p["bn1"][1]]


def _params(gpu):
    if "p" not in _CACHE:
        p = st.draw_params(700)
        _CACHE["p"] = (p, [_dev(gpu, a) for a in _plist(p)])
    return _CACHE["p"]


def _case(gpu, shape):
    key = ("case", shape)
    if key not in _CACHE:
        x, gp = st.draw_case(*shape, 3000 + sum(shape))
        _CACHE[key] = dict(x=x, gp=gp, dx=_dev(gpu, x), dgp=_dev(gpu, gp))
    return _CACHE[key]


def _forward(gpu, shape, cap=0):
    key = ("fwd", shape, cap)
    if key not in _CACHE:
        m = runtime.stem_train_forward(_case(gpu, shape)["dx"], _params(gpu)[1], st.EPS, max_chunk_pixels=cap)
        torch.cuda.synchronize()
        _CACHE[key] = (m, {k: v.cpu().numpy() for k, v in m.items()})
    return _CACHE[key]


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


def _grad(gpu, shape, want=(True,) * 4, cap=0, case=None, maps=None, params=None):
    c = case or _case(gpu, shape)
    m = maps or _forward(gpu, shape)[0]
    g = Guarded(gpu, OUT_SHAPES(*shape), want)
    dx, dp = runtime.stem_train_grad(c["dx"], m, c["dgp"], params or _params(gpu)[1], st.EPS, want_x=want[0],
                                     want_params=want[1:], out=(g.outs[0], g.outs[1:]), max_chunk_pixels=cap)
    torch.cuda.synchronize()
    assert g.intact(), "a guard band was written"
    return [None if t is None else t.cpu().numpy() for t in [dx] + list(dp)]


def _ratio(got, ref, bound):
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    assert np.isfinite(got).all(), "an element was not written"
    err, bound = np.abs(got - ref), np.broadcast_to(bound, np.shape(ref))
    exact = bound == 0
    assert not err[exact].any()
    return float(np.max(err[~exact] / bound[~exact])) if (~exact).any() else 0.0


def _forward_ratios(x, p, m, eps=st.EPS):
    """error / bound of every stage of the forward, each from the device's own inputs; a and pooled also bit for bit."""
    q = {}
    r, e = st.conv_stage(x, p["conv1"])
    q["z"] = _ratio(m["z"], r, e)
    (mean, var), (Em, Ev) = st.tr.stats_stage(m["z"])
    q["mean"], q["var"] = _ratio(m["stats"][0], mean, Em), _ratio(m["stats"][1], var, Ev)
    c = st.tr.coef(p["bn1"][0], p["bn1"][1], m["stats"][0], m["stats"][1], eps)
    a, Ea, _ = st.tr.apply_stage(m["z"], c)
    q["a"] = _ratio(m["a"], a, Ea)
    # one float32 FMA of the float32 pair, then the ReLU: s z is exact in float64, so one rounding of s z + t is the FMA
    s32, t32 = c[0].astype(np.float32), c[1].astype(np.float32)
    fma = (s32.astype(np.float64) * m["z"].astype(np.float64) + t32.astype(np.float64)).astype(np.float32)
    assert np.array_equal(m["a"], np.maximum(fma, np.float32(0)))
    assert np.array_equal(m["pooled"], st.pool(m["a"]).astype(np.float32))
    return q


def _grad_ratios(x, gp, p, m, got, Kc, eps=st.EPS):
    R, E = st.backward(x, m, gp, p, eps, Kc=Kc)
    return {k: _ratio(g, R[k], E[k]) for k, g in zip(st.GRADS, got) if g is not None}


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_stage_by_stage(gpu, shape, cap):
    p, _ = _params(gpu)
    c = _case(gpu, shape)
    _, m = _forward(gpu, shape, cap)
    q = _forward_ratios(c["x"], p, m)
    print(shape, "cap", cap, " ".join(f"{k} {v:.4f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q
    # the cap changes the order of the float64 sums only: z is the same bits
    assert np.array_equal(m["z"], _forward(gpu, shape, 0)[1]["z"])


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_on_the_stored_maps(gpu, shape, cap):
    p, _ = _params(gpu)
    c = _case(gpu, shape)
    _, m = _forward(gpu, shape)
    got = _grad(gpu, shape, cap=cap)
    Kc = runtime.stem_train_chunk_pixels(0, *shape, cap)
    n = shape[0] * m["z"].shape[1] * m["z"].shape[2]
    assert Kc == min(n, cap or 2048) and runtime.stem_train_chunk_pixels(1, *shape, cap) >= 1
    q = _grad_ratios(c["x"], c["gp"], p, m, got, Kc)
    print(shape, "cap", cap, "K_c", Kc, " ".join(f"{k} {v:.4f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q


def test_several_statistics_blocks_and_full_chunks(gpu):
    """What the table's last shape is there for."""
    assert runtime.stem_train_chunk_pixels(0, 2, 64, 96) == 2048
    n = 2 * 32 * 48
    assert -(-n // runtime.stem_train_chunk_pixels(1, 2, 64, 96)) > 1
    assert -(-n // runtime.stem_train_chunk_pixels(1, 2, 64, 96, 17)) > 1


@pytest.mark.parametrize("name", FIXTURE)
def test_reference_fixture(gpu, name):
    """The device on the fixture's image against the reference (torch on the CPU, float32, train()): z, a and pooled
    within the sum of the device's carried bound and the reference's, the same masks and window maxima; the gradient
    entry on the fixture's stored z, a and their float32 statistics against the reference's gradients within the sum
    of the device's bound and the reference's, both on those stored maps."""
    g = golden_io.load(GOLDEN, "stem_train_golden")
    p = dict(conv1=g["conv1.weight"], bn1=tuple(g[f"bn1.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))
    shape = FIXTURE[name]
    dps = [_dev(gpu, a) for a in _plist(p)]
    x, gp = g[f"{name}/x"], g[f"{name}/gp"]
    c = dict(dx=_dev(gpu, x), dgp=_dev(gpu, gp))
    m = {k: v.cpu().numpy() for k, v in runtime.stem_train_forward(c["dx"], dps, st.EPS).items()}
    V, E = st.forward_chain(x, p)
    _, E32 = st.forward_chain(x, p, f32=True)
    q = {k: _ratio(m[k], g[f"{name}/{k}"].astype(np.float64), E[k] + E32[k]) for k in ("z", "a", "pooled")}
    q["mean"], q["var"] = (_ratio(m["stats"][i], V["stats"][i], E["stats"][i]) for i in (0, 1))
    assert np.array_equal(m["a"] > 0, g[f"{name}/a"] > 0)
    assert np.array_equal(st.sr.pool_argmax(m["a"])[1], st.sr.pool_argmax(g[f"{name}/a"])[1])
    ref = dict(z=g[f"{name}/z"], a=g[f"{name}/a"], stats=np.array(st.tr.batch_stats(g[f"{name}/z"])).astype(np.float32))
    got = _grad(gpu, shape, case=c, maps={k: _dev(gpu, v) for k, v in ref.items()}, params=dps)
    R, Ed = st.backward(x, ref, gp, p, Kc=runtime.stem_train_chunk_pixels(0, *shape))
    _, Er = st.backward(x, ref, gp, p, f32=True)
    for k, gk, dv in zip(st.GRADS, ("dx", "conv1.weight.grad", "bn1.weight.grad", "bn1.bias.grad"), got):
        q[k] = _ratio(dv, g[f"{name}/{gk}"].astype(np.float64), Ed[k] + Er[k])
        q[k + " (device)"] = _ratio(dv, R[k], Ed[k])
    print(name, " ".join(f"{k} {v:.4f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q


def test_every_subset_of_outputs_and_bit_identical_runs(gpu):
    shape = (1, 6, 10)
    full = _grad(gpu, shape, cap=3)
    again = _grad(gpu, shape, cap=3)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    for want in itertools.product((False, True), repeat=4):
        if not any(want):
            continue
        got = _grad(gpu, shape, want=want, cap=3)
        for w, a, b in zip(want, got, full):
            assert (a is None) == (not w) and (a is None or np.array_equal(a, b))
    m1 = runtime.stem_train_forward(_case(gpu, shape)["dx"], _params(gpu)[1], st.EPS, max_chunk_pixels=3)
    m0 = _forward(gpu, shape, 3)[0]
    assert all(torch.equal(m0[k], m1[k]) for k in m0)


def test_graph_replay_matches_eager(gpu):
    shape = (2, 12, 20)
    c, (_, dps) = _case(gpu, shape), _params(gpu)
    eager_m = _forward(gpu, shape)[0]
    eager_g = _grad(gpu, shape)
    ash, psh = runtime.KfpnEngine.stem_shapes(*shape)
    out = {k: torch.full(s, float("nan"), device=gpu) for k, s in
           (("z", ash), ("a", ash), ("pooled", psh), ("stats", (2, 64)))}
    go = [torch.full(s, float("nan"), device=gpu) for s in OUT_SHAPES(*shape)]
    wf = torch.empty(runtime.stem_train_forward_workspace_bytes(*shape), dtype=torch.uint8, device=gpu)
    wg = torch.empty(runtime.stem_train_grad_workspace_bytes(*shape), dtype=torch.uint8, device=gpu)
    stream = torch.cuda.Stream(device=gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            runtime.stem_train_forward(c["dx"], dps, st.EPS, out=out, workspace=wf)
            runtime.stem_train_grad(c["dx"], out, c["dgp"], dps, st.EPS, out=(go[0], go[1:]), workspace=wg)
        for t in list(out.values()) + go:
            t.fill_(float("nan"))
        graph.replay()
    stream.synchronize()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager_m[k]) for k in out)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(go, eager_g))


def _raw(gpu, shape, run="fg", **over):
    """One raw call of each entry of ``run`` (f: forward, g: gradient) with sentinel-filled outputs; ``over`` replaces
    arguments.  Returns (rc forward, rc grad, outputs untouched); the code of an entry not run is None."""
    lib = _lib.lib()
    B, H, W = shape
    (ash, psh) = runtime.KfpnEngine.stem_shapes(max(B, 1), max(H, 1), max(W, 1))
    _, dps = _params(gpu)
    x = torch.zeros((max(B, 1), 3, max(H, 1), max(W, 1)), device=gpu)
    bufs = {k: torch.full(s, -7.25, device=gpu) for k, s in
            (("z", ash), ("a", ash), ("pooled", psh), ("stats", (2, 64)), ("gp", psh), ("dx", tuple(x.shape)),
             ("dW", (64, 3, 7, 7)), ("dg", (64,)), ("db", (64,)))}
    ws = torch.full((1 << 20,), 0, dtype=torch.uint8, device=gpu)
    a = dict(x=x.data_ptr(), params=(ctypes.c_void_p * 3)(*[t.data_ptr() for t in dps]), eps=st.EPS, cap=0,
             ws=ws.data_ptr(), ws_bytes=ws.numel(), **{k: v.data_ptr() for k, v in bufs.items()})
    a.update(over)
    sp = _lib.stream_ptr(gpu)
    rf = rg = None
    if "f" in run:
        rf = lib.sfa_stem_train_forward(a["x"], a["params"], a["eps"], B, H, W, a["z"], a["a"], a["pooled"], a["stats"],
                                        a["cap"], a["ws"], a["ws_bytes"], sp)
    dpar = (ctypes.c_void_p * 3)(a["dW"], a["dg"], a["db"])
    if "g" in run:
        rg = lib.sfa_stem_train_grad(a["x"], a["z"], a["a"], a["gp"], a["stats"], a["params"], a["eps"], B, H, W, a["dx"],
                                     dpar, a["cap"], a["ws"], a["ws_bytes"], sp)
    torch.cuda.synchronize()
    return rf, rg, all(bool((v == -7.25).all()) for v in bufs.values())


def test_refusals_leave_the_outputs_untouched(gpu):
    inv = INVALID
    ok = (1, 6, 10)
    cases = [((1, 1, 1), {}), ((1, 2, 2), {}), ((0, 6, 10), {}), ((1, 6, -1), {}), (ok, dict(eps=-1.0)), (ok, dict(cap=-1)),
             (ok, dict(ws_bytes=64)), (ok, dict(ws=None)), (ok, dict(params=None)), (ok, dict(stats=None)),
             (ok, dict(a=None)), (ok, dict(z=None))]
    for shape, over in cases:
        rf, rg, clean = _raw(gpu, shape, **over)
        assert rf == inv and rg == inv and clean, (shape, over, rf, rg)
    # misaligned buffers: 4 bytes into an allocation
    t = torch.zeros(64 * 3 * 7 * 7 + 4, device=gpu)
    for key in ("x", "z", "stats", "ws"):
        rf, rg, clean = _raw(gpu, ok, **{key: t.data_ptr() + 4})
        assert rf == inv and rg == inv and clean, key
    # what only the gradient reads, and no output wanted
    assert _raw(gpu, ok, run="g", gp=None)[1:] == (inv, True)
    assert _raw(gpu, ok, run="g", dx=None, dW=None, dg=None, db=None)[1:] == (inv, True)
    assert _raw(gpu, ok, run="g", x=None)[1:] == (inv, True)  # dW reads x
    # the size limits are SFA_E_UNSUPPORTED
    assert _raw(gpu, (65536, 3, 3), run="f")[0] == UNSUPPORTED
    for shape in ((1, 1, 1), (1, 2, 2), (0, 4, 4)):
        assert runtime.stem_train_forward_workspace_bytes(*shape) == 0 and runtime.stem_train_grad_workspace_bytes(*shape) == 0
        assert runtime.stem_train_chunk_pixels(0, *shape) == 0
    with pytest.raises(ValueError):
        runtime.stem_train_forward(torch.zeros((1, 3, 2, 2), device=gpu), _params(gpu)[1])
    # a size the fp16x3 stem operator refuses and this one takes: H above 32760
    assert runtime.stem_train_forward_workspace_bytes(1, 32762, 4) > 0
