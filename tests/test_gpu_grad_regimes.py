"""The gradient operators on the GPU at their plans' own chunk, block and pass regimes (tests/grad_regime_cases.py):
split-K with K_c = 2048 and a short last chunk, float64 partial blocks of more than 64 pixels, the heads' own
whole-row chunks, the stem data gradient's second pass and the workload's per-frame geometry.  Every row of the table
runs through the Python entry points against the float64 restatements within their derived bounds, computed for the
K_c the library reports (cross-checked against tools/grad_plan_dump.cpp).  Every run has NaN-prefilled outputs inside
guard bands and a workspace prefilled with NaN bytes, so a partial region that a short last chunk or block failed to
write cannot fold to a plausible number; a second run on a fresh workspace has to be bit-equal.  The engines, the
parameters and the helpers are those of the operators' own GPU tests."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest
import torch

import block_restatement as br
import block_train_restatement as tr
import grad_regime_cases as gc
import neck_restatement as nr
import stem_restatement as sr
import test_gpu_block as tb
import test_gpu_block_train as tt
import test_gpu_heads_grad as th
import test_gpu_neck as tn
import test_gpu_stem as ts
from sfa_hip import _lib, runtime

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Guarded = tb.Guarded


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """The dump's fields for every case of the table."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for tools/grad_plan_dump.cpp"
    exe = str(tmp_path_factory.mktemp("regimes") / "grad_plan_dump")
    r = subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(REPO, "tools", "grad_plan_dump.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    text = "\n".join(gc.query(c.op, c.args, c.shape, c.cap) for c in gc.CASES) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return [gc.parse(line) for line in r.stdout.splitlines()]


def _nan_bytes(gpu, nbytes):
    assert nbytes > 0
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)


def _host(ts_):
    return [None if t is None else t.cpu().numpy() for t in ts_]


def _twice(run):
    """run(nan_workspace) -> host arrays: once on a workspace of NaN bytes, once on a fresh one; bit-equal."""
    first, again = run(True), run(False)
    for a, b in zip(first, again):
        assert (a is None) == (b is None)
        assert a is None or np.array_equal(a.view(np.int32), b.view(np.int32)), "two runs differ"
    return first


def _block(gpu, c, f):
    layer, block = c.args
    B, h, w = c.shape
    eng = tb._engine(gpu)
    case = tb._case(gpu, layer, block, c.shape)
    d = case["dev"]
    shapes, ds = tb._shapes(layer, block, c.shape)
    want = [True] * 5 + [ds]
    kcs = [eng.block_grad_chunk_pixels(layer, block, which, B, h, w, c.cap) for which in (0, 1, 2)]
    assert kcs == [f["wg0.Kc"], f["wg1.Kc"], f["wg2.Kc"] if ds else 0], (kcs, f)
    need = eng.block_grad_workspace_bytes(layer, block, B, h, w, c.cap)
    assert need == f["total"]

    def run(nan):
        g = Guarded(gpu, shapes, want)
        dx, dp = eng.block_grad(layer, block, d["x"], d["mid"], d["y"], d["gy"], out=(g.outs[0], g.outs[1:]),
                                max_chunk_pixels=c.cap, workspace=_nan_bytes(gpu, need) if nan else None)
        torch.cuda.synchronize()
        assert g.intact(), "a guard band was written"
        return _host([dx] + list(dp))

    got = _twice(run)
    _, _, s, _ = br.block_shape(layer, block)
    R, E = br.backward(case["x"], case["mid"], case["y"], case["gy"], br.fold(tb._params(layer, block)), s, Kc=kcs[1])
    return {k: tb._ratio(g, R[k], E[k]) for k, g in zip(br.GRADS, got) if g is not None}


def _block_train(gpu, c, f):
    layer, block = c.args
    B, h, w = c.shape
    p, pd = tt._params(gpu, layer, block)
    case = tt._case(gpu, layer, block, c.shape)
    _, cout, s, ds = tr.block_shape(layer, block)
    kcs = [runtime.block_train_chunk_pixels(layer, block, which, B, h, w, c.cap) for which in (0, 1, 2, 3)]
    assert kcs == [f["wg0.Kc"], f["wg1.Kc"], f["wg2.Kc"] if ds else 0, f["st.pixels"]], (kcs, f)
    assert f["fst.pixels"] == f["st.pixels"]
    fneed = runtime.block_train_forward_workspace_bytes(layer, block, B, h, w, c.cap)
    gneed = runtime.block_train_grad_workspace_bytes(layer, block, B, h, w, c.cap)
    assert (fneed, gneed) == (f["f.total"], f["total"])
    names = ["z1", "mid", "z2"] + (["zd"] if ds else []) + ["y", "stats"]
    osh = (B, f["oh"], f["ow"], cout)

    def forward(nan):
        g = Guarded(gpu, [osh] * (len(names) - 1) + [(3 if ds else 2, 2, cout)], [True] * len(names))
        m = runtime.block_train_forward(layer, block, case["dx"], pd, tr.EPS, out=dict(zip(names, g.outs)),
                                        max_chunk_pixels=c.cap, workspace=_nan_bytes(gpu, fneed) if nan else None)
        torch.cuda.synchronize()
        assert g.intact(), "a guard band of the forward was written"
        forward.maps = m
        return _host([m[k] for k in names])

    mh = dict(zip(names, _twice(forward)))
    mh.setdefault("zd", None)
    for k, v in mh.items():
        assert v is None or np.isfinite(v).all(), k
    q = {"f:" + k: v for k, v in tt._forward_ratios(case["x"], p, s, mh).items()}
    maps = {k: (v.clone() if v is not None else None) for k, v in forward.maps.items()}  # out of the guarded storage
    shapes, _ = tt._out_shapes(layer, block, c.shape)

    def grad(nan):
        g = Guarded(gpu, shapes, [True] * len(shapes))
        outs = g.outs[1:] + [None] * (10 - len(shapes))
        dx, dp = runtime.block_train_grad(layer, block, case["dx"], maps, case["dgy"], pd, tr.EPS, out=(g.outs[0], outs),
                                          want_params=[True] * (len(shapes) - 1) + [False] * (10 - len(shapes)),
                                          max_chunk_pixels=c.cap, workspace=_nan_bytes(gpu, gneed) if nan else None)
        torch.cuda.synchronize()
        assert g.intact(), "a guard band of the gradient was written"
        return _host(([dx] + list(dp))[:len(shapes)])

    got = _twice(grad)
    R, E = tr.backward(case["x"], mh, case["gy"], p, s, Kc=kcs[1])
    keys = ["dx"] + list(tr.PARAMS[:9 if ds else 6])
    q.update({k: tt._ratio(g, R[k], E[k]) for k, g in zip(keys, got)})
    return q


def _neck(gpu, c, f):
    B, h4, w4 = c.shape
    eng, params = tn._engine(gpu)
    ls, gs = nr.draw_case(B, h4, w4, 900 + 100 * h4 + 10 * w4 + B)
    ld, gd = tn._dev(gpu, ls), tn._dev(gpu, gs)
    sh = eng._neck_shapes(B, h4, w4)
    us = eng.neck_forward(*ld)
    kc = [eng.neck_grad_chunk_pixels(k, B, h4, w4, c.cap) for k in (1, 2, 3)]
    assert kc == [f["wg1.Kc"], f["wg2.Kc"], f["wg3.Kc"]], (kc, f)
    need = eng.neck_grad_workspace_bytes(B, h4, w4, c.cap)
    assert need == f["total"]
    shapes = list(sh[:4]) + list(_lib.NECK_PARAM_SHAPES)

    def run(nan):
        g = Guarded(gpu, shapes, [True] * 10)
        dl, dp = eng.neck_grad(*gd, layers=ld, ups=us[:2], max_chunk_pixels=c.cap, out=(g.outs[:4], g.outs[4:]),
                               workspace=_nan_bytes(gpu, need) if nan else None)
        torch.cuda.synchronize()
        assert g.intact(), "a guard band was written"
        return _host(list(dl) + list(dp))

    got = _twice(run)
    R, E, _ = nr.backward(*ls, us[0].cpu().numpy(), us[1].cpu().numpy(), *gs, params, Kc=kc)
    return {k: tn._ratio(g, R[k], E[k]) for k, g in zip(tn.GRADS, got)}


def _stem(gpu, c, f):
    B, H, W = c.shape
    eng = ts._engine(gpu)
    case = ts._case(gpu, c.shape)
    d = case["dev"]
    kc = eng.stem_grad_chunk_pixels(B, H, W, c.cap)
    assert kc == f["wg.Kc"]
    need = eng.stem_grad_workspace_bytes(B, H, W, c.cap)
    assert need == f["total"]

    def run(nan):
        g = Guarded(gpu, [(B, 3, H, W), (64, 3, 7, 7), (64,)], [True] * 3)
        dx, dp = eng.stem_grad(d["x"], d["a"], d["gp"], out=(g.outs[0], g.outs[1:]), max_chunk_pixels=c.cap,
                               workspace=_nan_bytes(gpu, need) if nan else None)
        torch.cuda.synchronize()
        assert g.intact(), "a guard band was written"
        return _host([dx] + list(dp))

    got = _twice(run)
    R, E = sr.backward(case["x"], case["a"], case["gp"], sr.fold(ts.fixture_params())[0], Kc=kc)
    return {k: ts._ratio(g, R[k], E[k]) for k, g in zip(sr.GRADS, got)}


def _heads(gpu, c, f):
    level, (B, h, w) = c.args[0], c.shape
    eng, sd = th._engine(gpu)
    assert len(eng.heads) == gc.HEADS and th.CIN[level] == gc.LEVEL_CIN[level]
    x, g = th._inputs(eng, level, B, h, w, 100 * level + h * w)
    xd = torch.from_numpy(x).to(gpu)
    gd = {n: torch.from_numpy(v).to(gpu) for n, v in g.items()}
    kc = eng.heads_grad_chunk_pixels(level, B, h, w, c.cap)
    assert kc == f["Kc"]
    need = eng.heads_grad_workspace_bytes(level, B, h, w, c.cap)
    assert need == f["total"]
    shapes = [s for _, ch in eng.heads for s in ((64, th.CIN[level], 3, 3), (64,), (ch, 64, 1, 1), (ch,))]
    keep = {}

    def run(nan):
        gb = Guarded(gpu, shapes, [True] * len(shapes))
        out = {n: gb.outs[4 * j:4 * j + 4] for j, (n, _) in enumerate(eng.heads)}
        grads, hd, da = eng.heads_param_grad(level, xd, gd, out=out, want_hidden=True, max_chunk_pixels=c.cap,
                                             workspace=_nan_bytes(gpu, need) if nan else None)
        torch.cuda.synchronize()
        assert gb.intact(), "a guard band was written"
        keep["hd"], keep["da"] = hd.cpu().numpy(), da.cpu().numpy()
        return _host([t for n, _ in eng.heads for t in grads[n]]) + [keep["hd"], keep["da"]]

    flat = _twice(run)
    assert all(np.isfinite(a).all() for a in flat), "an element was not written"
    got = {n: flat[4 * j:4 * j + 4] for j, (n, _) in enumerate(eng.heads)}
    return th._check(eng, sd, level, x, g, got, keep["hd"], keep["da"], kc, gc.case_id(c))


RUN = {"block": _block, "block_train": _block_train, "neck": _neck, "stem": _stem, "heads": _heads}


@pytest.mark.parametrize("k", range(len(gc.CASES)), ids=[gc.case_id(c) for c in gc.CASES])
def test_case_within_the_derived_bounds(gpu, plans, k):
    c, f = gc.CASES[k], plans[k]
    assert f["ok"] == 1 and c.regimes - {"W"} <= gc.reached(f), (sorted(gc.reached(f)), f)
    for key, v in c.expect.items():
        assert f[key] == v, (key, f[key], v)
    t0 = time.time()
    q = RUN[c.op](gpu, c, f)
    print(f"grad regime {gc.case_id(c)} ({time.time() - t0:.1f} s): error / bound " +
          " ".join(f"{key} {v:.4f}" for key, v in q.items()))
    assert max(q.values()) <= 1.0, q
