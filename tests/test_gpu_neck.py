"""sfa_model_neck_forward and sfa_model_neck_grad on the GPU (csrc/neck.hip) against the numpy float64 restatement
(tests/neck_restatement.py) within the bounds derived there: every forward stage from the device's own inputs, all
ten gradients within the chained bound, the golden fixture's reference outputs, every NULL combination that changes
the launch set, one-hot known answers across the pixel tiles, overwrite, bit-identical runs, graph replay and every
error return."""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_io
import neck_restatement as nr
from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PNAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
GRADS = ("d_l1", "d_l2", "d_l3", "d_l4", "dW1", "db1", "dW2", "db2", "dW3", "db3")
_CACHE = {}


def _tile():
    return int(_lib.lib().sfa_neck_pixel_tile())


def _golden():
    if "golden" not in _CACHE:
        _CACHE["golden"] = golden_io.load(GOLDEN, "neck_golden")
    return _CACHE["golden"]


def _engine_with(gpu, key, params):
    if key not in _CACHE:
        arch = _lib.make_arch(dict(runtime.DEFAULT_HEADS))
        sd = dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), 11))
        for f in range(3):
            sd[f"conv_up_level{f + 1}.weight"] = params[2 * f].reshape(params[2 * f].shape + (1, 1)).copy()
            sd[f"conv_up_level{f + 1}.bias"] = params[2 * f + 1].copy()
        _CACHE[key] = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    return _CACHE[key]


def _engine(gpu):
    params = [_golden()[k] for k in PNAMES]
    return _engine_with(gpu, "eng", params), params


def _hot_params():
    """Weights with all values distinct and exact in float32 (multiples of 1 / 64), zero biases."""
    out = []
    for f, (co, cu, cs) in enumerate(zip(nr.COUT, nr.UP_C, nr.SKIP_C)):
        n = co * (cu + cs)
        rng = np.random.default_rng(50 + f)
        out += [((rng.permutation(n).astype(np.float32) - 0.5 * n) / 64.0).reshape(co, cu + cs), np.zeros(co, np.float32)]
    return out


def _shapes():
    """(B, h4, w4): the fixture's, 5 x 5, one frame of the smallest map, a level-3 pixel count that is no multiple of
    the tile where the tile allows one, the workload's 19 x 19.  A level-3 map has 64 B h4 w4 pixels, so with the
    tile of 64 that the library has today no shape gives the level-3 launches (d_l1, d_u3, u4, dW3) a short pixel
    tile: the search then falls back to (1, 1, 3), whose lower levels (3, 12 and 48 pixels) are all tile tails of
    the same kernels, and a short tile at level 3 itself stays unreached."""
    t = _tile()
    odd = next(((1, h, w) for h in range(1, 4) for w in range(1, 8) if (64 * h * w) % t), (1, 1, 3))
    return [(2, 1, 1), (2, 2, 3), (2, 3, 2), (2, 5, 5), (1, 1, 1), odd, (1, 19, 19)]


def _cap(B, h4, w4):
    n1 = 4 * B * h4 * w4
    return 3 if n1 < 9 else n1 // 3 + 1


def _dev(gpu, arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _ratio(got, ref, bound):
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all()
    return float(np.max(np.abs(got - ref) / bound))


def _case(gpu, shape):
    """One shape run once: inputs, the device's forward and full gradient (NaN-prefilled outputs), host copies."""
    key = ("case", shape)
    if key in _CACHE:
        return _CACHE[key]
    eng, params = _engine(gpu)
    B, h4, w4 = shape
    ls, gs = nr.draw_case(B, h4, w4, 900 + 100 * h4 + 10 * w4 + B)
    ld, gd = _dev(gpu, ls), _dev(gpu, gs)
    nan = lambda shapes: [torch.full(s, float("nan"), device=gpu) for s in shapes]  # noqa: E731
    sh = eng._neck_shapes(B, h4, w4)
    us = eng.neck_forward(*ld, out=nan(sh[4:]))
    cap = _cap(B, h4, w4)
    dl, dp = eng.neck_grad(*gd, layers=ld, ups=us[:2], max_chunk_pixels=cap,
                           out=(nan(sh[:4]), nan(_lib.NECK_PARAM_SHAPES)))
    torch.cuda.synchronize()
    res = dict(eng=eng, params=params, ls=ls, gs=gs, ld=ld, gd=gd, us=us, cap=cap, dl=dl, dp=dp,
               us_h=[t.cpu().numpy() for t in us], grads_h=[t.cpu().numpy() for t in dl + dp])
    _CACHE[key] = res
    return res


@pytest.mark.parametrize("case", range(7))
def test_forward_stage_by_stage(gpu, case):
    shape = _shapes()[case]
    c = _case(gpu, shape)
    W1, b1, W2, b2, W3, b3 = c["params"]
    l1, l2, l3, l4 = c["ls"]
    u2, u3, u4 = c["us_h"]
    q = [_ratio(u2, *nr.stage1(l4, l3, W1, b1)), _ratio(u3, *nr.stage2(u2, l2, W2, b2)),
         _ratio(u4, *nr.stage3(u3, l1, W3, b3))]
    print(f"neck forward {shape}: error / bound u2 {q[0]:.4f} u3 {q[1]:.4f} u4 {q[2]:.4f}")
    assert max(q) <= 1.0, q


@pytest.mark.parametrize("case", range(7))
def test_gradients_against_the_chained_bound(gpu, case):
    shape = _shapes()[case]
    c = _case(gpu, shape)
    eng, (B, h4, w4), cap = c["eng"], shape, c["cap"]
    kc = [eng.neck_grad_chunk_pixels(f, B, h4, w4, cap) for f in (1, 2, 3)]
    npix = [B * h4 * w4 << (2 * r) for r in range(4)]
    assert all(0 < k <= cap for k in kc)
    assert any(-(-n // cap) >= 3 and n % cap for n in npix[1:]), "no dW folds three chunks with a short last one"
    R, E, _ = nr.backward(*c["ls"], c["us_h"][0], c["us_h"][1], *c["gs"], c["params"], Kc=kc)
    q = {k: _ratio(g, R[k], E[k]) for k, g in zip(GRADS, c["grads_h"])}
    print(f"neck grad {shape} cap {cap}: error / bound " + " ".join(f"{k} {v:.4f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q


@pytest.mark.parametrize("name", ["B2_1x1", "B2_2x3", "B2_3x2"])
def test_reference_fixture(gpu, name):
    """The reference's stored outputs and gradients: device and reference each within their bound of the restatement,
    so within the sum of the two of each other."""
    g = _golden()
    assert name in list(g["cases"])
    eng, params = _engine(gpu)
    ls = [g[f"{name}/l{i}"] for i in (1, 2, 3, 4)]
    gs = [g[f"{name}/g{i}"] for i in (2, 3, 4)]
    ld, gd = _dev(gpu, ls), _dev(gpu, gs)
    us = eng.neck_forward(*ld)
    ref_us = _dev(gpu, [g[f"{name}/u2"], g[f"{name}/u3"]])
    dl, dp = eng.neck_grad(*gd, layers=ld, ups=ref_us)
    torch.cuda.synchronize()
    (_, _, _), Ef = nr.forward(*ls, params)
    for k, t, e in zip(("u2", "u3", "u4"), us, Ef):
        assert _ratio(t.cpu().numpy(), np.asarray(g[f"{name}/{k}"], np.float64), 2 * e) <= 1.0, k
    B = ls[3].shape[0]
    kc = [eng.neck_grad_chunk_pixels(f, B, ls[3].shape[1], ls[3].shape[2]) for f in (1, 2, 3)]
    _, Ed, _ = nr.backward(*ls, g[f"{name}/u2"], g[f"{name}/u3"], *gs, params, Kc=kc)
    _, Er, _ = nr.backward(*ls, g[f"{name}/u2"], g[f"{name}/u3"], *gs, params, f32=True)
    for k, t in zip(GRADS, dl + dp):
        ref = np.asarray(g[f"{name}/{k}"], np.float64)
        assert _ratio(t.cpu().numpy(), ref, Ed[k] + Er[k].reshape(Ed[k].shape)) <= 1.0, k


SUBSETS = {
    "no_params": ((True,) * 4, (False,) * 6),
    "no_layers": ((False,) * 4, (True,) * 6),
    "only_d_l1": ((True, False, False, False), (False,) * 6),
    "only_db2": ((False,) * 4, (False, False, False, True, False, False)),
    "only_d_l3": ((False, False, True, False), (False,) * 6),
    "only_dW1": ((False,) * 4, (True, False, False, False, False, False)),
    "only_d_l4": ((False, False, False, True), (False,) * 6),
    "dW3_db3": ((False,) * 4, (False, False, False, False, True, True)),
}


@pytest.mark.parametrize("which", sorted(SUBSETS))
def test_null_outputs_change_nothing_else(gpu, which):
    """Every subset of wanted outputs that changes the launch set gives the bits of the full run; the maps no wanted
    weight gradient reads are passed as NULL."""
    c = _case(gpu, (2, 2, 3))
    eng = c["eng"]
    wl, wp = SUBSETS[which]
    layers = list(c["ld"]) if any(wp[0::2]) else None
    ups = list(c["us"][:2]) if any(wp[0::2]) else None
    if which == "only_dW1":
        layers, ups = [None, None, c["ld"][2], c["ld"][3]], None
    dl, dp = eng.neck_grad(*c["gd"], layers=layers, ups=ups, want_layers=wl, want_params=wp, max_chunk_pixels=c["cap"])
    torch.cuda.synchronize()
    for got, full, want in zip(dl + dp, c["dl"] + c["dp"], wl + wp):
        assert (got is not None) == want
        if want:
            assert torch.equal(got.view(torch.int32), full.view(torch.int32))


def test_null_g2_g3_are_zero(gpu):
    c = _case(gpu, (2, 2, 3))
    eng = c["eng"]
    zeros = [torch.zeros_like(c["gd"][0]), torch.zeros_like(c["gd"][1])]
    for g2, g3 in ((None, c["gd"][1]), (c["gd"][0], None), (None, None)):
        a = eng.neck_grad(g2, g3, c["gd"][2], layers=c["ld"], ups=c["us"][:2])
        b = eng.neck_grad(zeros[0] if g2 is None else g2, zeros[1] if g3 is None else g3, c["gd"][2], layers=c["ld"],
                          ups=c["us"][:2])
        torch.cuda.synchronize()
        for x, y in zip(a[0] + a[1], b[0] + b[1]):  # x + 0 is x: the same bits
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    R, E, _ = nr.backward(*c["ls"], c["us_h"][0], c["us_h"][1], None, None, c["gs"][2], c["params"],
                          Kc=[eng.neck_grad_chunk_pixels(f, 2, 2, 3) for f in (1, 2, 3)])
    for k, t in zip(GRADS, a[0] + a[1]):
        assert _ratio(t.cpu().numpy(), R[k], E[k]) <= 1.0, k


def _hot_pixels(n):
    t = _tile()
    return sorted({0, n - 1, t - 1, t} & set(range(n)))


def test_one_hot_g4_gives_a_row_of_w3(gpu):
    """g4 = 1 at (pixel p, channel o): d_l1[p, :] = W3[o, 128:] exactly and zero elsewhere, at the first pixel, the
    last one and on both sides of the first pixel-tile edge."""
    P = _hot_params()
    eng = _engine_with(gpu, "hot", P)
    B, h4, w4 = 2, 1, 2
    n3 = 64 * B * h4 * w4
    assert n3 > _tile()
    for p in _hot_pixels(n3):
        for o in (0, 33, 63):
            g4 = np.zeros((n3, 64), np.float32)
            g4[p, o] = 1.0
            g4 = torch.from_numpy(g4.reshape(B, 8 * h4, 8 * w4, 64)).to(gpu)
            dl, _ = eng.neck_grad(None, None, g4, want_layers=(True, False, False, False), want_params=(False,) * 6)
            want = np.zeros((n3, 64), np.float32)
            want[p] = P[4][o, 128:]
            assert np.array_equal(dl[0].cpu().numpy().reshape(n3, 64), want), (p, o)


def test_one_hot_g3_gives_the_forward_coefficients(gpu):
    """g3 = 1 at one level-3 pixel and channel c, g4 = 0: dZ2 holds the (at most four) forward coefficients of that
    pixel, so d_l2[q, :] = float32(coefficient) * W2[c, 256:], one rounding, and zero at every other q."""
    P = _hot_params()
    eng = _engine_with(gpu, "hot", P)
    B, h4, w4 = 2, 1, 2
    H, W = 8 * h4, 8 * w4
    n3 = B * H * W
    for p in _hot_pixels(n3):
        c = (7 * p + 5) % 128
        g3 = np.zeros((n3, 128), np.float32)
        g3[p, c] = 1.0
        g3 = g3.reshape(B, H, W, 128)
        dz2 = nr.up_t(g3).astype(np.float32)  # products of two float32 coefficients: exact in float64, rounded once
        assert 1 <= np.count_nonzero(dz2) <= 4
        want = (dz2[..., c:c + 1].astype(np.float64) * P[2][c, 256:].astype(np.float64)).astype(np.float32)
        dl, _ = eng.neck_grad(None, torch.from_numpy(g3).to(gpu), torch.zeros((B, H, W, 64), device=gpu),
                              want_layers=(False, True, False, False), want_params=(False,) * 6)
        assert np.array_equal(dl[1].cpu().numpy(), want), p


def test_one_hot_degenerate_scale(gpu):
    """h4 = w4 = 1: U of the 1 x 1 map has scale 0, every output takes the single source with weight 1, so dL is the
    plain sum of dZ1 over its 2 x 2 pixels."""
    P = _hot_params()
    eng = _engine_with(gpu, "hot", P)
    g2 = np.zeros((1, 4, 4, 256), np.float32)
    g2[0, 3, 1, 9] = 1.0
    dz1 = nr.up_t(g2).astype(np.float32)
    dl = dz1.astype(np.float64).sum((1, 2)).astype(np.float32)  # at most four terms, added in float64, rounded once
    want = (dl[0, 9].astype(np.float64) * P[0][9, :512].astype(np.float64)).astype(np.float32)
    res, _ = eng.neck_grad(torch.from_numpy(g2).to(gpu), None, torch.zeros((1, 8, 8, 64), device=gpu),
                           want_layers=(False, False, False, True), want_params=(False,) * 6)
    assert np.array_equal(res[3].cpu().numpy().reshape(512), want)


def test_bit_identical_runs_and_graph_replay(gpu):
    c = _case(gpu, (2, 3, 2))
    eng, (B, h4, w4), cap = c["eng"], (2, 3, 2), c["cap"]
    sh = eng._neck_shapes(B, h4, w4)
    us2 = eng.neck_forward(*c["ld"])
    dl2, dp2 = eng.neck_grad(*c["gd"], layers=c["ld"], ups=c["us"][:2], max_chunk_pixels=cap)
    torch.cuda.synchronize()
    eager = list(c["us"]) + c["dl"] + c["dp"]
    for a, b in zip(eager, list(us2) + dl2 + dp2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    mk = lambda shapes: [torch.empty(s, device=gpu) for s in shapes]  # noqa: E731
    ous, odl, odp = mk(sh[4:]), mk(sh[:4]), mk(_lib.NECK_PARAM_SHAPES)
    wf = torch.empty(eng.neck_forward_workspace_bytes(B, h4, w4), dtype=torch.uint8, device=gpu)
    wg = torch.empty(eng.neck_grad_workspace_bytes(B, h4, w4, cap), dtype=torch.uint8, device=gpu)

    def run():
        eng.neck_forward(*c["ld"], out=ous, workspace=wf)
        eng.neck_grad(*c["gd"], layers=c["ld"], ups=ous[:2], out=(odl, odp), max_chunk_pixels=cap, workspace=wg)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        for t in ous + odl + odp:
            t.fill_(float("nan"))
        wf.fill_(0xFF)
        wg.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, ous + odl + odp):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_error_returns(gpu):
    eng, _ = _engine(gpu)
    L = _lib.lib()
    B, h4, w4 = 1, 1, 2
    sh = eng._neck_shapes(B, h4, w4)
    z = lambda shapes: [torch.zeros(s, device=gpu) for s in shapes]  # noqa: E731
    ls, us, gs, dls, dps = z(sh[:4]), z(sh[4:]), z(sh[4:]), z(sh[:4]), z(_lib.NECK_PARAM_SHAPES)
    nf, ng = eng.neck_forward_workspace_bytes(B, h4, w4), eng.neck_grad_workspace_bytes(B, h4, w4)
    assert nf > 0 and ng > 0
    wf = torch.empty(nf, dtype=torch.uint8, device=gpu)
    wg = torch.empty(ng, dtype=torch.uint8, device=gpu)
    sp = _lib.stream_ptr(gpu)
    P = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    arr = lambda v: (ctypes.c_void_p * 6)(*v)  # noqa: E731

    def fwd(model=eng._h, l=None, B=B, h4=h4, w4=w4, u=None, ws=wf.data_ptr(), nbytes=nf):
        return L.sfa_model_neck_forward(model, *(l or P(ls)), B, h4, w4, *(u or P(us)), ws, nbytes, sp)

    def grad(model=eng._h, l=None, u=None, g=None, B=B, h4=h4, w4=w4, d=None, dp=arr(P(dps)), cap=0, ws=wg.data_ptr(),
             nbytes=ng):
        return L.sfa_model_neck_grad(model, *(l or P(ls)), *(u or P(us[:2])), *(g or P(gs)), B, h4, w4, *(d or P(dls)), dp,
                                     cap, ws, nbytes, sp)

    assert fwd() == _lib.SFA_OK and grad() == _lib.SFA_OK
    torch.cuda.synchronize()
    inv, unsupported = -1, -2
    for call in (fwd, grad):
        assert call(model=None) == inv
        assert call(B=0) == inv and call(h4=0) == inv and call(w4=-2) == inv
        assert call(B=64, h4=64, w4=64) == inv  # offsets past 31 bits (nothing is read before the check)
        assert call(ws=None) == inv and call(ws=wf.data_ptr() + 4) == inv
    assert fwd(nbytes=nf - 1) == inv and grad(nbytes=ng - 1) == inv
    for i in range(4):
        bad = P(ls)
        bad[i] = None
        assert fwd(l=bad) == inv
        bad[i] = ls[i].data_ptr() + 4
        assert fwd(l=bad) == inv and grad(l=bad) == inv
    for i in range(3):
        bad = P(us)
        bad[i] = None
        assert fwd(u=bad) == inv
    assert grad(g=[gs[0].data_ptr(), gs[1].data_ptr(), None]) == inv  # g4 is required
    assert grad(g=[gs[0].data_ptr() + 8, gs[1].data_ptr(), gs[2].data_ptr()]) == inv
    assert grad(d=[None] * 4, dp=None) == inv and grad(d=[None] * 4, dp=arr([None] * 6)) == inv  # nothing wanted
    assert grad(cap=-1) == inv
    assert grad(u=[None, us[1].data_ptr()]) == inv and grad(l=[None] + P(ls)[1:]) == inv  # dW2 / dW3 need them
    assert grad(u=[None, None], l=[None] * 4, dp=None) == _lib.SFA_OK  # no dW wanted: the maps may be NULL
    assert eng.neck_forward_workspace_bytes(64, 64, 64) == 0 and eng.neck_grad_workspace_bytes(B, h4, w4, -1) == 0
    assert eng.neck_grad_chunk_pixels(0, B, h4, w4) == 0 and eng.neck_grad_chunk_pixels(4, B, h4, w4) == 0
    arch = _lib.make_arch(dict(runtime.DEFAULT_HEADS), backbone=_lib.BACKBONE_DECONV)
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 1)
    dec = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    assert fwd(model=dec._h) == unsupported and grad(model=dec._h) == unsupported
    assert L.sfa_model_neck_forward_workspace_size(dec._h, B, h4, w4) == 0
    with pytest.raises(ValueError):
        dec.neck_forward(*ls)
    torch.cuda.synchronize()
