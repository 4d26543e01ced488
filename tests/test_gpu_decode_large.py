"""The tiled decode (heat maps above 36,864 cells: sfa_decode / sfa_topk cut every class map into
tiles with a 1-cell halo, merge the tile lists per class, then per frame) against the CPU oracle,
bit for bit: selection is integer work on order-preserving keys and the gathers copy values, so
there is no tolerance anywhere.  On the parent commit every shape above 152 x 152 fails with
"decode: H*W = ... exceeds 36864".

Tile geometry at the shapes used (csrc/decode_plan.h tile_plan): 200 x 200 -> 10 tiles of 20 rows;
3 x 16384 -> 16 column tiles of 1024; 16384 x 3 -> 13 row tiles of 1261 rows; 1 x 40000 -> 40
column tiles of 1000; 512 x 512 -> 64 tiles of 8 rows (K = 256: 5 passes of the class merge).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import decode_oracle
from sfa_hip import _lib, runtime

pytestmark = pytest.mark.gpu

SCRIPTS = (2, 3, 200, 200, 50)      # the Argoverse scripts' configuration (800 x 800 input)
COLSPLIT = (1, 2, 3, 16384, 40)     # rows wider than a tile: column cuts with halo columns


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _aux(rng, B, H, W):
    return {k: rng.standard_normal((B, c, H, W)).astype(np.float32)
            for k, c in (("off", 2), ("dir", 2), ("z", 1), ("dim", 3))}


def _check(gpu, hm, aux, K, apply_sigmoid=False, with_off=True):
    off = aux["off"] if with_off else None
    got = runtime.decode(_t(hm, gpu), _t(off, gpu) if with_off else None, _t(aux["dir"], gpu), _t(aux["z"], gpu),
                         _t(aux["dim"], gpu), K=K, apply_sigmoid=apply_sigmoid).cpu().numpy()
    if apply_sigmoid:  # the oracle on the device's own sigmoid maps: the comparison stays exact
        hm = runtime.sigmoid_clamp_(_t(hm, gpu)).cpu().numpy()
        off = runtime.sigmoid_clamp_(_t(off, gpu)).cpu().numpy() if with_off else None
    exp = decode_oracle.decode(hm, off, aux["dir"], aux["z"], aux["dim"], K=K)
    np.testing.assert_array_equal(got, exp)
    return got


@pytest.mark.parametrize("B,C,H,W,K", [
    (1, 1, 193, 192, 50),      # the first size past the old limit
    SCRIPTS,
    COLSPLIT,
    (1, 2, 16384, 3, 40),      # many row tiles of a 3-column map
    (1, 1, 1, 40000, 7),       # one row: column tiles only, no row halo inside the map
    (1, 1, 512, 512, 256),     # the declared maximum with the largest K
    (1, 3, 152, 152, 50),      # at the old limit's side: still the band kernels, same entry
])
def test_decode_large_shapes_match_oracle(gpu, B, C, H, W, K):
    rng = np.random.default_rng(H * 7 + W + K)
    hm = rng.random((B, C, H, W), dtype=np.float32)
    _check(gpu, hm, _aux(rng, B, H, W), K)


def _tile_corners(H, W):
    """Cells at the corners of the tiles of an H x W map (and of the map), from the plan the header
    documents: rows cut evenly at <= 4096 / TC rows, columns at <= 1024."""
    nx = -(-W // 1024)
    tc = -(-W // nx)
    r = min(4096 // tc, 8192 // (tc + 2) - 2, H)
    ny = -(-H // r)
    r = -(-H // ny)
    ys = sorted({y for t in range(ny) for y in (t * r, min(H, t * r + r) - 1)})
    xs = sorted({x for t in range(nx) for x in (t * tc, min(W, t * tc + tc) - 1)})
    return ys, xs


@pytest.mark.parametrize("shape", [SCRIPTS, COLSPLIT])
@pytest.mark.parametrize("content", ["random", "sigmoid", "quantised", "constant", "negative", "isolated",
                                     "few_peaks", "no_offset"])
def test_decode_large_content(gpu, shape, content):
    B, C, H, W, K = shape
    rng = np.random.default_rng(len(content) * 100 + W)
    aux = _aux(rng, B, H, W)
    hm = rng.random((B, C, H, W), dtype=np.float32)
    if content == "random":
        _check(gpu, hm, aux, K)
    elif content == "sigmoid":  # logits, sigmoid + clamp fused into the tile pass (and on the offsets)
        _check(gpu, (rng.standard_normal((B, C, H, W)) * 3).astype(np.float32), aux, K, apply_sigmoid=True)
    elif content == "quantised":  # 7 levels: plateaus and ties across every tile edge and corner
        _check(gpu, (np.floor(hm * 7) / 7).astype(np.float32), aux, K)
    elif content == "constant":  # every cell a peak: indices 0 .. K-1 of class 0
        got = _check(gpu, np.full((B, C, H, W), 0.25, np.float32), aux, K)
        assert np.all(got[..., 9] == 0)
        np.testing.assert_array_equal(got[0, :, 3], aux["z"][0, 0].reshape(-1)[:K])
    elif content == "negative":  # non-peaks become zeros and outrank every (negative) peak
        _check(gpu, -hm - np.float32(0.5), aux, K)
    elif content == "isolated":  # lone peaks on tile corners and the map border, over a flat floor
        m = np.full((B, C, H, W), 0.001, np.float32)
        ys, xs = _tile_corners(H, W)
        v = 0.5
        for y in ys:
            for x in xs:
                m[:, :, y, x] = np.float32(v)
                v += 0.001
        _check(gpu, m, aux, K)
    elif content == "few_peaks":  # fewer than K peaks: the rest of the K are zeros, lowest index first
        m = np.zeros((B, C, H, W), np.float32)
        for j in range(5):
            m[:, :, (j * 37) % H, (j * 911) % W] = np.float32(0.3 + 0.1 * j)
        _check(gpu, m, aux, K)
    else:
        _check(gpu, hm, aux, K, with_off=False)


@pytest.mark.parametrize("ties", [False, True])
def test_topk_large_matches_oracle(gpu, ties):
    B, C, H, W, K = SCRIPTS
    n = B * C * H * W
    s = (np.random.default_rng(9).permutation(n).astype(np.float32) / n).reshape(B, C, H, W)
    if ties:
        s = (np.round(s * 64) / 64).astype(np.float32)
    sc, ind, cls, ys, xs = (t.cpu().numpy() for t in runtime.topk(_t(s, gpu), K))
    for got, exp in zip((sc, ind, cls, ys, xs), decode_oracle.topk(s, K)):
        np.testing.assert_array_equal(got, exp)
    csc, cind, cys, cxs = (t.cpu().numpy() for t in runtime.topk(_t(s, gpu), K, per_channel=True))
    flat = s.reshape(B, C, H * W)
    for b in range(B):
        for c in range(C):
            v, i = decode_oracle._topk_desc(flat[b, c], K)
            np.testing.assert_array_equal(csc[b, c], v)
            np.testing.assert_array_equal(cind[b, c], i)
            np.testing.assert_array_equal(cys[b, c], (i // W).astype(np.float32))
            np.testing.assert_array_equal(cxs[b, c], (i % W).astype(np.float32))


def test_decode_large_in_a_graph(gpu):
    """Captured once, replayed on changed maps: the tiled form allocates nothing, keeps no state
    between runs and leaves nothing in its workspace that the next run relies on."""
    B, C, H, W, K = SCRIPTS
    rng = np.random.default_rng(21)
    aux = _aux(rng, B, H, W)
    dev = {k: _t(v, gpu) for k, v in aux.items()}
    hm = torch.zeros((B, C, H, W), dtype=torch.float32, device=gpu)
    out = torch.empty((B, K, 10), dtype=torch.float32, device=gpu)
    dec = runtime.Decoder()
    ws = torch.empty(dec.workspace_bytes(B, C, K, H, W), dtype=torch.uint8, device=gpu)

    def run():
        dec(hm, dev["off"], dev["dir"], dev["z"], dev["dim"], K=K, out=out, workspace=ws)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for seed in (1, 2):
        m = np.random.default_rng(seed).random((B, C, H, W), dtype=np.float32)
        hm.copy_(_t(m, gpu))
        g.replay()
        exp = decode_oracle.decode(m, aux["off"], aux["dir"], aux["z"], aux["dim"], K=K)
        np.testing.assert_array_equal(out.cpu().numpy(), exp)


def test_decode_large_argument_errors(gpu):
    """Too small a workspace is SFA_E_WORKSPACE, a map above 512 x 512 cells SFA_E_INVALID, both
    decided on the host before any launch (the output stays as it was)."""
    L = _lib.lib()
    B, C, H, W, K = 1, 3, 200, 200, 50
    need = L.sfa_decode_workspace_size_hw(B, C, H, W, K)
    maps = torch.zeros((B, 11, H, W), dtype=torch.float32, device=gpu)
    out = torch.full((B, K, 10), 7.0, dtype=torch.float32, device=gpu)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    p = maps.data_ptr()
    args = (p, p, p, p, p, B, C, H, W, K, 0, out.data_ptr(), ws.data_ptr())
    assert L.sfa_decode(*args, need - 1, None) == -4
    assert b"workspace" in L.sfa_last_error_string()
    assert L.sfa_decode(*args, need // 2, None) == -4
    big = (p, p, p, p, p, B, C, 513, 512, K, 0, out.data_ptr(), ws.data_ptr())
    assert L.sfa_decode(*big, need, None) == -1
    assert b"exceeds 262144" in L.sfa_last_error_string()
    i64 = ctypes.c_void_p(out.data_ptr())
    assert L.sfa_topk(p, B, C, H, W, K, 0, i64, i64, i64, i64, i64, ws.data_ptr(), need - 1, None) == -4
    assert L.sfa_topk(p, B, C, 513, 512, K, 0, i64, i64, i64, i64, i64, ws.data_ptr(), need, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(_lib.SfaNativeError, match="exceeds 262144"):
        runtime.decode(torch.zeros((1, 1, 513, 512), device=gpu), None, torch.zeros((1, 2, 513, 512), device=gpu),
                       torch.zeros((1, 1, 513, 512), device=gpu), torch.zeros((1, 3, 513, 512), device=gpu), K=10)
