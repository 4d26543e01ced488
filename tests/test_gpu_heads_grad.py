"""sfa_model_heads_grad on the GPU (csrc/heads_grad.hip): the parameter gradients of one KFPN level's heads
against the numpy float64 restatement (tests/heads_grad_restatement.py), evaluated from the very Hd and dA the
kernels used, within the bounds derived there; known answers, chunkings, bit-identical runs, graph replay and
every error return."""
import ctypes

import numpy as np
import pytest
import torch

import heads_grad_restatement as hr
from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

CIN = _lib.HEADS_LEVEL_CIN
SHAPES = [(2, 6, 8), (2, 5, 7), (2, 1, 1), (2, 1, 9)]
CHUNKINGS = (0, 7, 1)
ARCHS = {"five": dict(runtime.DEFAULT_HEADS), "two": {"a": 2, "b": 1}}
_CACHE = {}


def _engine(gpu, which="five"):
    key = ("eng", which)
    if key not in _CACHE:
        arch = _lib.make_arch(ARCHS[which])
        sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 11)
        _CACHE[key] = (runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu), sd)
    return _CACHE[key]


def _inputs(eng, level, B, h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, h, w, CIN[level])).astype(np.float32)
    g = {n: rng.standard_normal((B, c, h, w)).astype(np.float32) for n, c in eng.heads}
    return x, g


def _run(eng, level, x, g, mcp=0, **kw):
    dev = eng.device
    xd = torch.from_numpy(x).to(dev)
    gd = {n: torch.from_numpy(v).to(dev) for n, v in g.items()}
    res = eng.heads_param_grad(level, xd, gd, want_hidden=True, max_chunk_pixels=mcp, **kw)
    torch.cuda.synchronize()
    grads, hd, da = res
    return {n: [t.cpu().numpy() for t in v] for n, v in grads.items()}, hd.cpu().numpy(), da.cpu().numpy()


def _params(sd, level, name):
    pre = f"fpn{level}_{name}"
    return [np.asarray(sd[f"{pre}.{k}"], np.float32) for k in ("0.weight", "0.bias", "2.weight", "2.bias")]


def _check(eng, sd, level, x, g, got, hd, da, Kc, what):
    """Every output of one run against the restatement; returns the worst ratios."""
    B, h, w, _ = x.shape
    npix = B * h * w
    worst = {}
    for j, (name, c) in enumerate(eng.heads):
        W1, b1, W2, b2 = _params(sd, level, name)
        sl = slice(64 * j, 64 * j + 64)
        _, Hd_ref, _ = hr.forward(x, W1, b1, W2, b2)
        gq, ok = hr.gate(hd[..., sl], Hd_ref)
        print(f"{what} {name}: Hd gate {gq:.3e}")
        assert ok, (what, name, "Hd", gq)
        dA_ref, _ = hr.dhidden(hd[..., sl], W2, g[name])
        ref = hr.grads(x, hd[..., sl], W2, g[name], dA32=da[..., sl])
        dW1, db1, dW2, db2 = got[name]
        ratios = {
            "dA": hr.worst_ratio(da[..., sl], dA_ref, hr.bound_dA(dA_ref)),
            "dW1": hr.worst_ratio(dW1, ref["dW1"], hr.bound_dW1(ref["dW1"], ref["S_dW1"], Kc, npix)),
            "db1": hr.worst_ratio(db1, ref["db1"], hr.bound_f64_sum(ref["db1"], ref["S_db1"], npix)),
            "dW2": hr.worst_ratio(dW2.reshape(c, 64), ref["dW2"], hr.bound_f64_sum(ref["dW2"], ref["S_dW2"], npix)),
            "db2": hr.worst_ratio(db2, ref["db2"], hr.bound_f64_sum(ref["db2"], ref["S_db2"], npix)),
        }
        print(f"{what} {name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        for k, v in ratios.items():
            assert v <= 1.0, (what, name, k, v)
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("level", [0, 1, 2])
def test_small_maps_all_chunkings(gpu, level, shape):
    eng, sd = _engine(gpu)
    B, h, w = shape
    x, g = _inputs(eng, level, B, h, w, 100 * level + h * w)
    runs = {}
    for mcp in CHUNKINGS:
        Kc = eng.heads_grad_chunk_pixels(level, B, h, w, mcp)
        assert Kc == max(1, min(h, (mcp or 4096) // w)) * w
        got, hd, da = _run(eng, level, x, g, mcp)
        assert not any(np.isnan(a).any() for v in got.values() for a in v)
        _check(eng, sd, level, x, g, got, hd, da, Kc, f"L{level} {shape} mcp={mcp}")
        runs[mcp] = (got, hd, da, Kc)
    base = runs[0]
    for mcp in CHUNKINGS[1:]:
        got, hd, da, Kc = runs[mcp]
        assert np.array_equal(hd, base[1]) and np.array_equal(da, base[2])
        for name in got:
            for k in (1, 2, 3):  # db1, dW2, db2 do not depend on the chunking
                assert np.array_equal(got[name][k], base[0][name][k]), (mcp, name, k)
            if Kc == base[3]:  # equal chunkings: the same bits
                assert np.array_equal(got[name][0], base[0][name][0]), (mcp, name)
    if runs[7][3] == runs[1][3]:
        for name in runs[7][0]:
            assert np.array_equal(runs[7][0][name][0], runs[1][0][name][0])


def test_level2_full_map(gpu):
    eng, sd = _engine(gpu)
    B, h, w = 2, 152, 152
    x, g = _inputs(eng, 2, B, h, w, 7)
    Kc = eng.heads_grad_chunk_pixels(2, B, h, w, 0)
    assert Kc == (4096 // 152) * 152
    got, hd, da = _run(eng, 2, x, g, 0)
    _check(eng, sd, 2, x, g, got, hd, da, Kc, "L2 152x152")


def test_other_arch(gpu):
    eng, sd = _engine(gpu, "two")
    x, g = _inputs(eng, 1, 2, 5, 7, 3)
    for mcp in (0, 7):
        got, hd, da = _run(eng, 1, x, g, mcp)
        assert hd.shape == (2, 5, 7, 128)
        _check(eng, sd, 1, x, g, got, hd, da, eng.heads_grad_chunk_pixels(1, 2, 5, 7, mcp), f"two-head mcp={mcp}")


# (2, 3, 37): an odd width above the kernel's 32-pixel LDS segment; the hot pixel at columns 31 and 32 takes its
# left / right neighbour from the other segment's halo column, and the second segment is a 5-pixel odd tail
@pytest.mark.parametrize("level,shape,pos", [(2, (2, 5, 7), (1, 0, 0)), (1, (2, 5, 7), (0, 4, 6)),
                                             (0, (2, 5, 7), (1, 2, 3)), (2, (2, 3, 37), (1, 1, 31)),
                                             (2, (2, 3, 37), (0, 1, 32)), (1, (2, 3, 37), (1, 2, 36))])
def test_one_hot_known_answer(gpu, level, shape, pos):
    """W1 = 0 and b1 = 1 make Hd = 1 everywhere; W2 of one head one-hot at (0, o0) and g one-hot at channel 0 of one
    pixel make dA one-hot: dW1[o0] is then a shifted copy of x, exactly, and everything else is zero."""
    arch = _lib.make_arch(ARCHS["five"])
    sd = {k: np.zeros_like(v) if k.startswith("fpn") else v
          for k, v in synthetic.synthetic_state_dict(_lib.state_layout(arch), 11).items()}
    j0, o0 = 3, 37
    names = [n for n in ARCHS["five"]]
    for f in range(3):
        for n in names:
            sd[f"fpn{f}_{n}.0.bias"] = np.ones(64, np.float32)
    sd[f"fpn{level}_{names[j0]}.2.weight"][0, o0, 0, 0] = 1.0
    eng = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    B, h, w = shape
    b0, y0, x0 = pos
    x, dA, want = hr.one_hot_case(B, h, w, CIN[level], 64, b0, y0, x0, o0, seed=level)
    g = {n: np.zeros((B, c, h, w), np.float32) for n, c in eng.heads}
    g[names[j0]][b0, 0, y0, x0] = 1.0
    for mcp in CHUNKINGS:
        got, hd, da = _run(eng, level, x, g, mcp)
        assert np.array_equal(hd, np.ones_like(hd))
        assert np.array_equal(da[..., 64 * j0:64 * j0 + 64], dA) and np.count_nonzero(da) == 1
        for j, n in enumerate(names):
            assert np.array_equal(got[n][0], want if j == j0 else np.zeros_like(want)), (mcp, n)
            assert np.array_equal(got[n][1], dA[b0, y0, x0] if j == j0 else np.zeros(64, np.float32))


def test_bit_identical_runs_and_graph_replay(gpu):
    eng, _ = _engine(gpu)
    level, B, h, w = 1, 2, 6, 8
    x, g = _inputs(eng, level, B, h, w, 5)
    xd = torch.from_numpy(x).to(gpu)
    gd = {n: torch.from_numpy(v).to(gpu) for n, v in g.items()}
    first = eng.heads_param_grad(level, xd, gd, max_chunk_pixels=7)
    second = eng.heads_param_grad(level, xd, gd, max_chunk_pixels=7)
    torch.cuda.synchronize()
    for n in first:
        for a, b in zip(first[n], second[n]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    out = {n: [torch.empty_like(t) for t in v] for n, v in first.items()}
    ws = torch.empty(eng.heads_grad_workspace_bytes(level, B, h, w, 7), dtype=torch.uint8, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.heads_param_grad(level, xd, gd, out=out, max_chunk_pixels=7, workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.heads_param_grad(level, xd, gd, out=out, max_chunk_pixels=7, workspace=ws)
    for v in out.values():
        for t in v:
            t.fill_(float("nan"))
    ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    for n in first:
        for a, b in zip(first[n], out[n]):
            assert not torch.isnan(b).any()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), n


def test_error_returns(gpu):
    eng, _ = _engine(gpu)
    L = _lib.lib()
    level, B, h, w = 2, 1, 4, 4
    x = torch.zeros((B, h, w, 64), device=gpu)
    g = [torch.zeros((B, c, h, w), device=gpu) for _, c in eng.heads]
    outs = [[torch.empty(s, device=gpu) for _ in eng.heads] for s in ((64, 64, 3, 3), (64,), (4, 64), (4,))]
    need = eng.heads_grad_workspace_bytes(level, B, h, w)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    sp = _lib.stream_ptr(gpu)

    def call(model=eng._h, level=level, x=x.data_ptr(), B=B, h=h, w=w, g=arr(g), o=None, mcp=0, ws=ws.data_ptr(),
             nbytes=need, hid=None):
        o = o or [arr(t) for t in outs]
        return L.sfa_model_heads_grad(model, level, x, B, h, w, g, *o, hid, None, mcp, ws, nbytes, sp)

    assert call() == _lib.SFA_OK
    torch.cuda.synchronize()
    inv, wsp = -1, -4
    assert call(model=None) == inv
    assert call(level=3) == inv and call(level=-1) == inv
    assert call(x=None) == inv
    assert call(B=0) == inv and call(h=0) == inv and call(w=-2) == inv
    assert call(mcp=-1) == inv
    assert call(g=None) == inv
    assert call(ws=None) == inv
    null_head = arr(g)
    null_head[2] = None
    assert call(g=null_head) == inv
    for k in range(4):
        o = [arr(t) for t in outs]
        o[k][1] = None
        assert call(o=o) == inv
    assert call(x=x.data_ptr() + 4) == inv  # misaligned
    assert call(nbytes=need - 1) == wsp
    # offsets past 32 bits: B h w 320 4 >= 2^31 (nothing is read before the check)
    assert call(B=64, h=512, w=512) == inv
    assert eng.heads_grad_workspace_bytes(level, 64, 512, 512) == 0
    assert eng.heads_grad_workspace_bytes(3, B, h, w) == 0 and eng.heads_grad_chunk_pixels(level, 0, h, w) == 0
    # the plain resnet_18 family has no KFPN head levels
    arch = _lib.make_arch(ARCHS["five"], backbone=_lib.BACKBONE_DECONV)
    sd = synthetic.synthetic_state_dict(_lib.state_layout(arch), 1)
    dec = runtime.KfpnEngine(arch, runtime.pack_state_dict(sd, arch), gpu)
    assert call(model=dec._h) == -2
    torch.cuda.synchronize()
