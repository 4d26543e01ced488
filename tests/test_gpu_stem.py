"""sfa_model_stem_forward and sfa_model_stem_grad on the GPU (csrc/stem_grad.hip) against the numpy float64 restatement
(tests/stem_restatement.py) within the bounds derived there: a one-pixel pooled map, odd conv and pooled maps, a pixel
count that is no multiple of the 64-pixel tile, the two chain cases, split-K caps 0, 3 and 17, the first-maximum known
answers, every combination of wanted outputs with guard bands, the reference fixture, bit-identical runs, graph replay,
the forward at the per-stage gate and every error return."""
import ctypes

import numpy as np
import pytest
import torch

import stem_restatement as sr
from sfa_hip import _lib, runtime, synthetic
from test_stem_host import CASES as FIXTURE_CASES
from test_stem_host import PARAMS, fixture, fixture_params, nhwc, pool_known_answers

pytestmark = pytest.mark.gpu

_CACHE = {}
GUARD = 64  # floats on either side of every output buffer
SHAPES = [(1, 4, 4), (1, 6, 10), (2, 12, 20), (1, 36, 52), (2, 64, 96), (1, 32, 160)]
CAPS = (0, 3, 17)
MAX_SIDE = 32760  # include/sfa_hip.h: the largest accepted H and W


def _engine(gpu, deconv=False):
    """An engine whose stem is the fixture's (both backbone families pack it alike)."""
    key = ("eng", deconv)
    if key not in _CACHE:
        arch = _lib.make_arch(dict(runtime.DEFAULT_HEADS), backbone=_lib.BACKBONE_DECONV) if deconv else \
            _lib.make_arch(dict(runtime.DEFAULT_HEADS))
        sd = dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), 11))
        p = fixture_params()
        sd["conv1.weight"] = p["conv1"].copy()
        for k, v in zip(("weight", "bias", "running_mean", "running_var"), p["bn1"]):
            assert sd[f"bn1.{k}"].shape == v.shape
            sd[f"bn1.{k}"] = v.copy()
        _CACHE[key] = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    return _CACHE[key]


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _case(gpu, shape):
    key = ("case", shape)
    if key not in _CACHE:
        c = sr.draw_case(*shape, 7000 + sum(shape))
        c["dev"] = {k: _dev(gpu, c[k]) for k in ("x", "a", "gp")}
        _CACHE[key] = c
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


def _grad(gpu, shape, want=(True, True, True), cap=0, maps=None, eng=None):
    eng = eng or _engine(gpu)
    d = maps or _case(gpu, shape)["dev"]
    B, H, W = shape
    g = Guarded(gpu, [(B, 3, H, W), (64, 3, 7, 7), (64,)], want)
    dx, dp = eng.stem_grad(d["x"], d["a"], d["gp"], want_x=want[0], want_params=want[1:], out=(g.outs[0], g.outs[1:]),
                           max_chunk_pixels=cap)
    torch.cuda.synchronize()
    assert g.intact(), "a guard band was written"
    return [None if t is None else t.cpu().numpy() for t in [dx] + list(dp)]


def _ratio(got, ref, bound):
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), "an element was not written"
    return sr.ratio(got, ref, bound)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_at_the_stage_gate(gpu, shape):
    """a and pooled within 1e-5 max(1, |v|) of the restatement; pooled bit-equal to the max-pool of the device's a."""
    eng = _engine(gpu)
    c = _case(gpu, shape)
    a, pooled = eng.stem_forward(c["dev"]["x"])
    torch.cuda.synchronize()
    a, pooled = a.cpu().numpy(), pooled.cpu().numpy()
    Wf, bf = sr.fold(fixture_params())
    ra, rp = sr.forward(c["x"], Wf, bf)
    q = [float(np.max(np.abs(g - r) / np.maximum(1.0, np.abs(r)))) for g, r in ((a, ra), (pooled, rp))]
    print(f"stem forward {shape}: a {q[0]:.3e} pooled {q[1]:.3e}")
    assert a.shape == ra.shape and pooled.shape == rp.shape and max(q) <= 1e-5, q
    assert np.array_equal(pooled.astype(np.float64), sr.pool_argmax(a)[0])
    # the deconv family's handle packs the same stem: the same bits
    a2, p2 = _engine(gpu, deconv=True).stem_forward(c["dev"]["x"])
    assert np.array_equal(a2.cpu().numpy(), a) and np.array_equal(p2.cpu().numpy(), pooled)


@pytest.mark.parametrize("shape", [(2, 64, 96), (1, 32, 160)])
def test_forward_against_the_models_unfused_stem(gpu, shape):
    """No stage view exposes the model's pooled map, so the comparison is one stage later: layer1 of the model's own
    forward with SFA_OPT_STEM_PATCH off against layer1.0 and layer1.1 (sfa_model_block_forward) on this operator's
    pooled map, within the 2e-5 that tests/test_gpu_model.py test_stem_patch_matches_gather_stem allows."""
    eng = _engine(gpu)
    B, H, W = shape
    x = _case(gpu, shape)["dev"]["x"]
    _, pooled = eng.stem_forward(x)
    _, y = eng.block_forward(1, 0, pooled)
    _, y = eng.block_forward(1, 1, y)
    old = eng.get_option(_lib.OPT_STEM_PATCH)
    eng.set_option(_lib.OPT_STEM_PATCH, 0)
    try:
        ws = eng.workspace(B, H, W)
        eng.forward_into(x, eng.alloc_outputs(B, H, W), _lib.IN_NCHW3, ws)
        torch.cuda.synchronize()
        mine = eng.debug_views(ws, B, H, W)["layer1"].permute(0, 2, 3, 1).cpu().numpy()
    finally:
        eng.set_option(_lib.OPT_STEM_PATCH, old)
    y = y.cpu().numpy()
    q = float(np.max(np.abs(y - mine) / np.maximum(1.0, np.abs(mine))))
    print(f"stem + layer1 against the model's own {shape}: {q:.3e} (bit-equal: {np.array_equal(y, mine)})")
    assert q <= 2e-5


@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_within_the_derived_bounds(gpu, shape):
    eng = _engine(gpu)
    c = _case(gpu, shape)
    Wf, _ = sr.fold(fixture_params())
    for cap in CAPS:
        kc = eng.stem_grad_chunk_pixels(*shape, cap)
        assert kc >= 1 and (cap == 0 or kc <= cap)
        R, E = sr.backward(c["x"], c["a"], c["gp"], Wf, Kc=kc)
        got = dict(zip(sr.GRADS, _grad(gpu, shape, cap=cap)))
        q = {k: _ratio(got[k], R[k], E[k]) for k in sr.GRADS}
        print(f"stem grad {shape} cap {cap} (K_c {kc}): error / bound " + " ".join(f"{k} {v:.4f}" for k, v in q.items()))
        assert max(q.values()) <= 1.0, q


def test_gradients_on_the_devices_own_map(gpu):
    """The forward's own a (not a drawn one) feeds the gradient: the restatement reads the very same map."""
    shape = (1, 36, 52)
    eng = _engine(gpu)
    c = _case(gpu, shape)
    a, _ = eng.stem_forward(c["dev"]["x"])
    maps = dict(x=c["dev"]["x"], a=a, gp=c["dev"]["gp"])
    got = dict(zip(sr.GRADS, _grad(gpu, shape, maps=maps)))
    R, E = sr.backward(c["x"], a.cpu().numpy(), c["gp"], sr.fold(fixture_params())[0], Kc=eng.stem_grad_chunk_pixels(*shape))
    q = {k: _ratio(got[k], R[k], E[k]) for k in sr.GRADS}
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("name,a,gp,want", pool_known_answers(), ids=lambda v: v if isinstance(v, str) else "")
def test_pool_adjoint_known_answers_on_the_device(gpu, name, a, gp, want):
    """The one-hot cases of tests/test_stem_host.py on the device, read back through db' (the channel sums of dA) and
    through dW' against an all-ones image (per tap, the sum of dA over the cells whose tap lies inside the image):
    sums of small integers, so both are exact and together pin down where dA landed."""
    B, oh, ow, _ = a.shape
    H, W = 2 * oh, 2 * ow
    x = torch.ones((B, 3, H, W), device=gpu)
    maps = dict(x=x, a=_dev(gpu, a), gp=_dev(gpu, gp))
    dx, dW, db = _grad(gpu, (B, H, W), maps=maps)
    assert np.array_equal(db, want.reshape(-1, 64).sum(0))
    # with x = 1 inside the image, dW'[o][c][ky][kx] sums dA over the cells whose tap lies inside: an exact integer sum
    R, _ = sr.backward(np.ones((B, 3, H, W), np.float32), a, gp, sr.fold(fixture_params())[0])
    assert np.array_equal(np.where(a > 0, sr.pool_adjoint(a, gp)[0], 0.0), want.astype(np.float64))
    assert np.array_equal(dW.astype(np.float64), R["dW"])


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("shape", [(1, 6, 10), (1, 36, 52)])
def test_wanted_outputs_and_repetition_are_bit_exact(gpu, shape):
    full = _grad(gpu, shape, cap=17)
    again = _grad(gpu, shape, cap=17)
    assert all(_bits(a, b) for a, b in zip(full, again))
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        part = _grad(gpu, shape, want=want, cap=17)
        for wnt, p, f in zip(want, part, full):
            assert (p is None) == (not wnt) and (p is None or _bits(p, f)), want
    # dW' alone does not need x's gradient buffer, dx and db' alone do not need x
    eng = _engine(gpu)
    d = _case(gpu, shape)["dev"]
    B, H, W = shape
    need = eng.stem_grad_workspace_bytes(B, H, W, 17)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    gx, db = torch.empty((B, 3, H, W), device=gpu), torch.empty(64, device=gpu)
    arr = (ctypes.c_void_p * 2)(None, db.data_ptr())
    assert _lib.lib().sfa_model_stem_grad(eng._h, None, d["a"].data_ptr(), d["gp"].data_ptr(), B, H, W, gx.data_ptr(), arr,
                                          17, ws.data_ptr(), need, _lib.stream_ptr(gpu)) == 0
    torch.cuda.synchronize()
    assert _bits(gx.cpu().numpy(), full[0]) and _bits(db.cpu().numpy(), full[2])


def test_graph_replay_equals_the_eager_run(gpu):
    shape = (1, 36, 52)
    eng = _engine(gpu)
    d = _case(gpu, shape)["dev"]
    B, H, W = shape
    eager = _grad(gpu, shape)
    ash, psh = eng.stem_shapes(B, H, W)
    a, pooled = torch.empty(ash, device=gpu), torch.empty(psh, device=gpu)
    outs = (torch.empty((B, 3, H, W), device=gpu), [torch.empty((64, 3, 7, 7), device=gpu), torch.empty(64, device=gpu)])
    fws = torch.empty(eng.stem_forward_workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)
    gws = torch.empty(eng.stem_grad_workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)
    ea, ep = eng.stem_forward(d["x"])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            eng.stem_forward(d["x"], out=(a, pooled), workspace=fws)
            eng.stem_grad(d["x"], d["a"], d["gp"], out=outs, workspace=gws)
    for t in (a, pooled, outs[0], *outs[1]):
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, ea) and torch.equal(pooled, ep)
    assert all(_bits(t.cpu().numpy(), e) for t, e in zip([outs[0]] + outs[1], eager))


@pytest.mark.parametrize("case", FIXTURE_CASES)
def test_reference_fixture(gpu, case):
    """The reference's stem (tests/golden/stem_golden.npz) on its own stored maps: sfa_model_stem_grad then
    sfa_bn_unfold_grad within the device's bound of the restatement, the reference within its float32 bound of it, so
    the two within the sum of the bounds of each other, element by element; and the forward at the stage gate."""
    g, p = fixture(), fixture_params()
    eng = _engine(gpu)
    m = dict(x=g[f"{case}/x"], a=nhwc(g[f"{case}/a"]), gp=nhwc(g[f"{case}/gp"]))
    d = {k: _dev(gpu, v) for k, v in m.items()}
    B, _, H, W = m["x"].shape
    dx, dp = eng.stem_grad(d["x"], d["a"], d["gp"], max_chunk_pixels=17)
    gam, _, mu, var = p["bn1"]
    got = {"dx": dx}
    got["conv1.weight"], got["bn1.weight"], got["bn1.bias"] = runtime.bn_unfold_grad(
        _dev(gpu, p["conv1"]), _dev(gpu, gam), _dev(gpu, mu), _dev(gpu, var), sr.EPS, dp[0], dp[1])
    fa, fp = eng.stem_forward(d["x"])
    torch.cuda.synchronize()
    for t, r in ((fa, m["a"]), (fp, nhwc(g[f"{case}/pooled"]))):
        assert float(np.max(np.abs(t.cpu().numpy() - r) / np.maximum(1.0, np.abs(r)))) <= 2e-5  # both sides' 1e-5
    kc = eng.stem_grad_chunk_pixels(B, H, W, 17)
    R, E = sr.unfolded(p, m["x"], m["a"], m["gp"], Kc=kc)
    _, Eref = sr.unfolded(p, m["x"], m["a"], m["gp"], f32=True)
    q = {}
    for k, t in got.items():
        dev = t.cpu().numpy().astype(np.float64).reshape(R[k].shape)
        ref = g[f"{case}/{k}" + ("" if k == "dx" else ".grad")]
        q[k] = (sr.ratio(dev, R[k], E[k]), sr.ratio(ref, R[k], Eref[k]),
                sr.ratio(dev, ref.astype(np.float64).reshape(R[k].shape), E[k] + Eref[k]))
    print(f"stem fixture {case}: (device, reference, device - reference) / bound " +
          " ".join(f"{k} {a:.4f} {b:.4f} {c:.4f}" for k, (a, b, c) in q.items()))
    assert set(got) == {"dx"} | set(PARAMS) and max(max(v) for v in q.values()) <= 1.0, q


def test_refusals(gpu):
    L = _lib.lib()
    eng = _engine(gpu)
    B, H, W = 2, 12, 20
    d = _case(gpu, (B, H, W))["dev"]
    SENT = -7.25
    outs = [torch.full(s, SENT, device=gpu) for s in ((B, 3, H, W), (64, 3, 7, 7), (64,))]
    need = eng.stem_grad_workspace_bytes(B, H, W)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=gpu)
    sp = _lib.stream_ptr(gpu)

    def grad(x=d["x"].data_ptr(), a=d["a"].data_ptr(), gp=d["gp"].data_ptr(), B=B, H=H, W=W, gx=outs[0].data_ptr(),
             dp="all", cap=0, wsp=ws.data_ptr(), nb=need, m=eng._h):
        if dp == "all":
            dp = [t.data_ptr() for t in outs[1:]]
        arr = None if dp is None else (ctypes.c_void_p * 2)(*dp)
        return L.sfa_model_stem_grad(m, x, a, gp, B, H, W, gx, arr, cap, wsp, nb, sp)

    inv, uns = -1, -2  # SFA_E_INVALID, SFA_E_UNSUPPORTED
    for kw in (dict(m=None), dict(a=None), dict(gp=None), dict(wsp=None), dict(x=None), dict(B=0), dict(H=0), dict(W=-1),
               dict(cap=-1), dict(nb=need - 1), dict(gx=None, dp=None), dict(gx=None, dp=[None, None]),
               dict(gx=outs[0].data_ptr() + 4), dict(wsp=ws.data_ptr() + 4), dict(gp=d["gp"].data_ptr() + 8),
               dict(B=32, H=1024, W=1024)):
        assert grad(**kw) == inv, kw
    for kw in (dict(H=MAX_SIDE + 1), dict(W=MAX_SIDE + 1), dict(B=65536, H=2, W=2)):
        assert grad(**kw) == uns, kw
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs), "a refused call wrote an output"
    assert grad() == 0
    assert eng.stem_grad_workspace_bytes(B, H, W, -1) == 0 and eng.stem_grad_chunk_pixels(B, H, MAX_SIDE + 1) == 0
    assert eng.stem_forward_workspace_bytes(1, MAX_SIDE + 1, 4) == 0 and eng.stem_forward_workspace_bytes(1, MAX_SIDE, 4) > 0
    # forward: the same argument checks; the largest accepted side runs (H = 32760 at W = 4: a 16380 x 2 conv map)
    fneed = eng.stem_forward_workspace_bytes(B, H, W)
    fws = torch.empty(fneed, dtype=torch.uint8, device=gpu)
    ash, psh = eng.stem_shapes(B, H, W)
    ao, po = torch.full(ash, SENT, device=gpu), torch.full(psh, SENT, device=gpu)
    fwd = lambda x=d["x"].data_ptr(), B=B, H=H, W=W, nb=fneed, m=eng._h, wsp=fws.data_ptr(), a=ao.data_ptr(): \
        L.sfa_model_stem_forward(m, x, B, H, W, a, po.data_ptr(), wsp, nb, sp)  # noqa: E731
    for kw in (dict(m=None), dict(x=None), dict(a=None), dict(H=0), dict(B=-1), dict(nb=fneed - 1), dict(wsp=None),
               dict(x=d["x"].data_ptr() + 4), dict(B=32, H=1024, W=1024)):
        assert fwd(**kw) == inv, kw
    for kw in (dict(H=MAX_SIDE + 1), dict(W=MAX_SIDE + 1), dict(B=65536)):
        assert fwd(**kw) == uns, kw
    torch.cuda.synchronize()
    assert bool((ao == SENT).all()) and bool((po == SENT).all())
    assert fwd() == 0
    with pytest.raises(ValueError):
        eng.stem_forward(torch.zeros((1, 4, 8, 8), device=gpu))
    torch.cuda.synchronize()


def test_largest_accepted_side(gpu):
    """H = 32760, the edge of the accepted set, against the restatement at the stage gate."""
    eng = _engine(gpu)
    rng = np.random.default_rng(9)
    x = rng.standard_normal((1, 3, MAX_SIDE, 4)).astype(np.float32)
    a, pooled = eng.stem_forward(_dev(gpu, x))
    torch.cuda.synchronize()
    Wf, bf = sr.fold(fixture_params())
    ra, rp = sr.forward(x, Wf, bf)
    for g, r in ((a.cpu().numpy(), ra), (pooled.cpu().numpy(), rp)):
        assert g.shape == r.shape and float(np.max(np.abs(g - r) / np.maximum(1.0, np.abs(r)))) <= 1e-5
