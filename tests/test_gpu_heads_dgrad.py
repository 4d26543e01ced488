"""sfa_model_heads_input_grad and sfa_model_heads_forward on the GPU (csrc/heads_grad.hip): the heads' input gradient
against the numpy float64 restatement (tests/heads_dgrad_restatement.py) evaluated from the device's own dA, within
the bound derived there; one-hot known answers across the kernel's pixel tiles; the forward's y from the device's own
Hd, and that Hd against the parameter-gradient entry's; bit-identical runs, graph replay and every error return."""
import ctypes

import numpy as np
import pytest
import torch

import heads_dgrad_restatement as dr
import heads_grad_restatement as hr
from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

CIN = _lib.HEADS_LEVEL_CIN
ARCHS = {"five": dict(runtime.DEFAULT_HEADS), "two": {"a": 2, "b": 1}}
_CACHE = {}


def _tile():
    return _lib.heads_dgrad_pixel_tile()


def _engine(gpu, which="five"):
    key = ("eng", which)
    if key not in _CACHE:
        arch = _lib.make_arch(ARCHS[which])
        sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 11)
        _CACHE[key] = (runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu), sd)
    return _CACHE[key]


def _w1_all(eng, sd, level):
    return np.concatenate([np.asarray(sd[f"fpn{level}_{n}.0.weight"], np.float32) for n, _ in eng.heads], axis=0)


def _device_dA(eng, level, B, h, w, seed):
    """x, g and the dA / Hd that sfa_model_heads_grad leaves for them (device tensors and host copies)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, h, w, CIN[level])).astype(np.float32)
    g = {n: torch.from_numpy(rng.standard_normal((B, c, h, w)).astype(np.float32)).to(eng.device) for n, c in eng.heads}
    xd = torch.from_numpy(x).to(eng.device)
    _, hd, da = eng.heads_param_grad(level, xd, g, want_hidden=True)
    return x, xd, hd, da


def _ratio(eng, sd, level, B, h, w, seed, what):
    _, _, _, da = _device_dA(eng, level, B, h, w, seed)
    got = eng.heads_input_grad(level, da)
    torch.cuda.synchronize()
    got, da = got.cpu().numpy(), da.cpu().numpy()
    assert got.shape == (B, h, w, CIN[level]) and not np.isnan(got).any()
    ref, S = dr.dgrad(da, _w1_all(eng, sd, level))
    q = hr.worst_ratio(got, ref, dr.bound_dX(ref, S, da.shape[3]))
    print(f"{what}: dX error / bound {q:.4f}, gate {hr.gate(got, ref)[0]:.3e}")
    return q


def _shapes():
    t = _tile()
    return [(2, 6, 8), (2, 5, 7), (2, 1, 1), (2, 1, 9), (2, 1, t + 1), (2, 1, t - 1)]


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("level", [0, 1, 2])
def test_error_against_the_bound(gpu, level, case):
    eng, sd = _engine(gpu)
    B, h, w = _shapes()[case]
    assert _ratio(eng, sd, level, B, h, w, 100 * level + h * w, f"L{level} {(B, h, w)}") <= 1.0


def test_other_arch(gpu):
    eng, sd = _engine(gpu, "two")
    _, _, _, da = _device_dA(eng, 1, 2, 5, 7, 3)
    assert da.shape == (2, 5, 7, 128)
    assert _ratio(eng, sd, 1, 2, 5, 7, 3, "two-head L1 5x7") <= 1.0


def test_level2_full_map(gpu):
    eng, sd = _engine(gpu)
    assert 152 > 2 * _tile() or 152 % _tile()  # several tiles per row and a row tail
    assert _ratio(eng, sd, 2, 1, 152, 152, 7, "L2 152x152") <= 1.0


def _one_hot_engine(gpu, level):
    key = ("hot", level)
    if key not in _CACHE:
        arch = _lib.make_arch(ARCHS["five"])
        sd = dict(synthetic.synthetic_state_dict(_lib.state_layout(arch), 11))
        W1, _, _ = dr.one_hot_case(1, 1, 1, CIN[level], 320, 0, 0, 0, 0, seed=level)
        for j, n in enumerate(ARCHS["five"]):
            sd[f"fpn{level}_{n}.0.weight"] = W1[64 * j:64 * j + 64].copy()
        _CACHE[key] = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    return _CACHE[key]


def _one_hot_maps():
    t = _tile()
    return {"37": ((2, 3, 37), [(0, 0, 0), (1, 2, 36), (1, 1, 31), (0, 1, 32), (1, 0, 36)]),
            "two_tiles_plus_5": ((1, 2, 2 * t + 5), [(0, 0, t - 1), (0, 1, t), (0, 1, 2 * t + 4)])}


@pytest.mark.parametrize("which", ["37", "two_tiles_plus_5"])
@pytest.mark.parametrize("level", [2, 1])
def test_one_hot_known_answer(gpu, level, which):
    """dA = 1 at one (b, y0, x0, o0): dX is W1[o0, :, ky, kx] at (y0 + ky - 1, x0 + kx - 1), exactly, the taps that
    leave the map absent, everything else zero; hot pixels on both sides of a pixel-tile edge and in the row tail."""
    eng = _one_hot_engine(gpu, level)
    (B, h, w), hots = _one_hot_maps()[which]
    for b0, y0, x0 in hots:
        for o0 in (0, 63, 319):
            _, dA, want = dr.one_hot_case(B, h, w, CIN[level], 320, b0, y0, x0, o0, seed=level)
            got = eng.heads_input_grad(level, torch.from_numpy(dA).to(gpu)).cpu().numpy()
            assert np.array_equal(got, want), (level, which, (b0, y0, x0), o0)


@pytest.mark.parametrize("level,shape", [(0, (2, 5, 7)), (1, (2, 6, 8)), (2, (2, 1, 9))])
def test_heads_forward(gpu, level, shape):
    eng, sd = _engine(gpu)
    B, h, w = shape
    x, xd, hd_grad, _ = _device_dA(eng, level, B, h, w, 40 + level)
    ys, hd = eng.heads_forward(level, xd, want_hidden=True)
    torch.cuda.synchronize()
    assert torch.equal(hd.view(torch.int32), hd_grad.view(torch.int32))  # the same kernels on the same bits
    hd = hd.cpu().numpy()
    for j, (n, c) in enumerate(eng.heads):
        W1, b1, W2, b2 = (np.asarray(sd[f"fpn{level}_{n}.{k}"], np.float32)
                          for k in ("0.weight", "0.bias", "2.weight", "2.bias"))
        _, Hd_ref, _ = hr.forward(x, W1, b1, W2, b2)
        gq, ok = hr.gate(hd[..., 64 * j:64 * j + 64], Hd_ref)
        assert ok, (n, "Hd", gq)
        ref, mag = dr.head_out(hd[..., 64 * j:64 * j + 64], W2, b2)
        got = ys[n].cpu().numpy()
        assert got.shape == (B, c, h, w) and not np.isnan(got).any()
        q = hr.worst_ratio(got, ref, dr.bound_y(ref, mag))
        print(f"L{level} {shape} {n}: Hd gate {gq:.3e}, y error / bound {q:.4f}")
        assert q <= 1.0, (n, q)


def test_bit_identical_runs_and_graph_replay(gpu):
    eng, _ = _engine(gpu)
    level, B, h, w = 1, 2, 3, _tile() + 5
    _, xd, _, da = _device_dA(eng, level, B, h, w, 5)
    first, second = eng.heads_input_grad(level, da), eng.heads_input_grad(level, da)
    y1 = eng.heads_forward(level, xd)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    out = torch.empty_like(first)
    yout = {n: torch.empty_like(t) for n, t in y1.items()}
    ws = torch.empty(eng.heads_forward_workspace_bytes(level, B, h, w), dtype=torch.uint8, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.heads_input_grad(level, da, out=out)
        eng.heads_forward(level, xd, out=yout, workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.heads_input_grad(level, da, out=out)
        eng.heads_forward(level, xd, out=yout, workspace=ws)
    for _ in range(2):
        out.fill_(float("nan"))
        for t in yout.values():
            t.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(first.view(torch.int32), out.view(torch.int32))
        for n in y1:
            assert torch.equal(y1[n].view(torch.int32), yout[n].view(torch.int32)), n


def test_error_returns(gpu):
    eng, _ = _engine(gpu)
    L = _lib.lib()
    level, B, h, w = 2, 1, 4, 4
    da = torch.zeros((B, h, w, 320), device=gpu)
    gx = torch.empty((B, h, w, 64), device=gpu)
    x = torch.zeros((B, h, w, 64), device=gpu)
    ys = [torch.empty((B, c, h, w), device=gpu) for _, c in eng.heads]
    need = eng.heads_forward_workspace_bytes(level, B, h, w)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    sp = _lib.stream_ptr(gpu)

    def dgrad(model=eng._h, level=level, da=da.data_ptr(), B=B, h=h, w=w, gx=gx.data_ptr()):
        return L.sfa_model_heads_input_grad(model, level, da, B, h, w, gx, sp)

    def fwd(model=eng._h, level=level, x=x.data_ptr(), B=B, h=h, w=w, y=arr(ys), hid=None, ws=ws.data_ptr(), nbytes=need):
        return L.sfa_model_heads_forward(model, level, x, B, h, w, y, hid, ws, nbytes, sp)

    assert dgrad() == _lib.SFA_OK and fwd() == _lib.SFA_OK
    torch.cuda.synchronize()
    inv, unsupported, wsp = -1, -2, -4
    for call in (dgrad, fwd):
        assert call(model=None) == inv
        assert call(level=3) == inv and call(level=-1) == inv
        assert call(B=0) == inv and call(h=0) == inv and call(w=-2) == inv
        assert call(B=64, h=512, w=512) == inv  # offsets past 32 bits (nothing is read before the check)
    assert dgrad(da=None) == inv and dgrad(gx=None) == inv
    assert dgrad(da=da.data_ptr() + 4) == inv and dgrad(gx=gx.data_ptr() + 8) == inv  # misaligned
    assert fwd(x=None) == inv and fwd(y=None) == inv and fwd(ws=None) == inv
    null_head = arr(ys)
    null_head[2] = None
    assert fwd(y=null_head) == inv
    assert fwd(x=x.data_ptr() + 4) == inv and fwd(hid=x.data_ptr() + 4) == inv and fwd(ws=ws.data_ptr() + 4) == inv
    assert fwd(nbytes=need - 1) == wsp
    assert eng.heads_forward_workspace_bytes(level, 64, 512, 512) == 0 and eng.heads_forward_workspace_bytes(3, B, h, w) == 0
    # the plain resnet_18 family has no KFPN head levels
    arch = _lib.make_arch(ARCHS["five"], backbone=_lib.BACKBONE_DECONV)
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 1)
    dec = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    assert dgrad(model=dec._h) == unsupported and fwd(model=dec._h) == unsupported
    torch.cuda.synchronize()
