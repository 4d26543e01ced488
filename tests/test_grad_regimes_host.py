"""The host proof of the gradient regime table (tests/grad_regime_cases.py), from the output of
tools/grad_plan_dump.cpp (its own main, built with ASan + UBSan; no preloading) and not from a restated formula:
every case reaches the regimes it claims; the cases of the operators' own GPU tests reach none of them (with the two
exceptions recorded below); every case is the smallest of its kind within its search box; and, on the CPU, a
restatement-side mutant of the mistake each regime guards against exceeds the very bound the GPU test holds the
kernels to."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import block_restatement as br
import grad_regime_cases as gc
import heads_grad_restatement as hr
import stem_restatement as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "grad_plan_dump.cpp")
NEW = ("S", "Sf", "O", "Ps", "Pf", "Ph", "R", "G")  # S16 is what the stem's own test already reaches


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("regimes") / "grad_plan_dump")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def ask(queries):
        r = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(queries)
        return [gc.parse(line) for line in lines]

    return ask


def _fields(dump, c):
    return dump([gc.query(c.op, c.args, c.shape, c.cap)])[0]


def test_every_case_reaches_what_it_claims(dump):
    fs = dump([gc.query(c.op, c.args, c.shape, c.cap) for c in gc.CASES])
    for c, f in zip(gc.CASES, fs):
        assert f["ok"] == 1, c
        got = gc.reached(f)
        assert c.regimes - {"W"} <= got, (gc.case_id(c), sorted(got))
        for key, v in c.expect.items():
            assert f[key] == v, (gc.case_id(c), key, f[key], v)
        print(gc.case_id(c), "reaches", sorted(got), {k: f[k] for k in f if k.endswith((".Kc", ".chunks", ".last", ".pixels",
              ".blocks", "_chunk", "_frame", "_rows", ".passes"))})
    ops = {(c.op, r) for c in gc.CASES for r in c.regimes}
    for want in [("block", "S"), ("block", "Sf"), ("block", "O"), ("block", "Ps"), ("block", "Pf"), ("block", "W"),
                 ("block_train", "S"), ("block_train", "O"), ("block_train", "Ps"), ("block_train", "Pf"),
                 ("block_train", "W"), ("neck", "S"), ("stem", "S"), ("stem", "Ps"), ("stem", "G"), ("heads", "Ph"),
                 ("heads", "R"), ("heads", "W")]:
        assert want in ops, want
    assert {c.args for c in gc.CASES if c.op == "heads" and "R" in c.regimes} == {(0,), (1,), (2,)}
    assert {c.args for c in gc.CASES if c.op == "block" and "S" in c.regimes} == {(L, 1) for L in (1, 2, 3, 4)} | \
        {(L, 0) for L in (2, 3, 4)}


def test_the_operators_own_tables_reach_none_of_them(dump):
    """The record of the gap: the shapes and caps of tests/test_gpu_block.py, test_gpu_block_train.py, test_gpu_stem.py
    and test_gpu_heads_grad.py, read from those modules.  Two regimes were reached before and are recorded as such:
    the stem's (2, 64, 96) splits at cap 0 with a tail of 1024 pixels, a whole number of LDS steps (S16, never S); and
    test_gpu_heads_grad.py test_level2_full_map runs level 2 at (2, 152, 152) with cap 0, which has the plan's own
    row chunks and long hidden-gradient blocks (R and Ph), at level 2 only: levels 0 and 1 never ran the plan's own
    cut."""
    import test_gpu_block as tb
    import test_gpu_block_train as tt
    import test_gpu_heads_grad as th
    import test_gpu_stem as ts
    old = [("block", (L, b), s, cap) for L, b, s in tb.CASES for cap in tb.CAPS]
    old += [("block_train", (L, b), s, cap) for L, b, s in tt.CASES for cap in tt.CAPS]
    old += [("stem", (), s, cap) for s in ts.SHAPES for cap in ts.CAPS]
    old += [("heads", (lv,), s, cap) for lv in (0, 1, 2) for s in th.SHAPES for cap in th.CHUNKINGS]
    fs = dump([gc.query(*o) for o in old])
    for o, f in zip(old, fs):
        assert f["ok"] == 1, o
        assert not gc.reached(f) & set(NEW), (o, sorted(gc.reached(f)))
        assert o[2][1:] != (152, 152), o
    assert any("S16" in gc.reached(f) for o, f in zip(old, fs) if o[0] == "stem")
    full = dump([gc.query("heads", (2,), (2, 152, 152), 0)])[0]
    assert gc.reached(full) == {"R", "Ph"}
    assert any(c.op == "heads" and c.args != (2,) and "R" in c.regimes for c in gc.CASES)


def _box(c):
    primary = next((r for r in ("G", "Sf", "S", "Ps", "Pf", "Ph", "R") if r in c.regimes), None)
    name = c.op
    if c.op in ("block", "block_train"):
        name = "block2" if c.args[1] == 0 else "block"
    return primary, gc.BOXES.get((name, primary))


def _size(f, primary):
    """What "smaller" means: the pixels the regime's sums run over, then the pixels of the input."""
    if f["op"] in ("block", "block_train"):
        return (f["npix_out"], f["npix_in"])
    if f["op"] == "neck":
        return (f["npix0"],)
    if f["op"] == "stem":
        return (f["npix_x"],) if primary == "G" else (f["npix_a"], f["npix_x"])
    return (f["B"] * f["h"] * f["w"],)


def test_every_case_is_the_smallest_of_its_kind(dump):
    seen = {}
    for c in gc.CASES:
        if c.regimes == {"W"}:
            continue  # a statement about one shape
        primary, box = _box(c)
        assert box is not None, gc.case_id(c)
        B, (h0, h1), (w0, w1) = box
        assert B == c.shape[0] and h0 <= c.shape[1] <= h1 and w0 <= c.shape[2] <= w1, gc.case_id(c)
        key = (c.op, c.args[1:] if c.op != "heads" else (), primary, tuple(sorted(c.regimes)))
        if key not in seen:  # the plans' geometry does not depend on the layer or the level
            shapes = [(B, h, w) for h in range(h0, h1 + 1) for w in range(w0, w1 + 1)]
            fs = dump([gc.query(c.op, c.args, s, c.cap) for s in shapes])
            hits = [(_size(f, primary), s) for s, f in zip(shapes, fs) if f["ok"] and c.regimes <= gc.reached(f)]
            seen[key] = min(hits)
        best = seen[key]
        mine = _size(_fields(dump, c), primary)
        print(gc.case_id(c), "size", mine, "smallest in the box", best)
        assert (mine, c.shape) == best, (gc.case_id(c), mine, best)


# ---- mutants: the restatement's own sums with the mistake a regime guards against, against the GPU test's bound

def _runs(n, per):
    return [(i, min(per, n - i)) for i in range(0, n, per)]


def _wgrad_mutants(d2, x2, Kc):
    """dz^T x with the last chunk dropped, and with the last chunk read at the first chunk's offset."""
    runs = _runs(d2.shape[0], Kc)
    assert len(runs) >= 2 and runs[-1][1] < Kc
    first, count = runs[-1]
    head = d2[:first].T @ x2[:first]
    return head, head + d2[:count].T @ x2[:count]


def _worst(got, ref, bound):
    return br.ratio(got, ref, bound)


def _report(what, factors):
    print(f"mutant {what}: error / bound " + " ".join(f"{k} {v:.3g}" for k, v in factors.items()))
    assert min(factors.values()) > 1.0, (what, factors)


@pytest.mark.parametrize("layer,block", [(1, 1), (2, 0)])
def test_split_k_mutants_of_a_block(dump, layer, block):
    c = next(c for c in gc.CASES if c.op == "block" and c.args == (layer, block) and "S" in c.regimes)
    f = _fields(dump, c)
    _, cout, s, _ = br.block_shape(layer, block)
    m = br.draw_case(layer, block, *c.shape, 1)
    R, E = br.backward(m["x"], m["mid"], m["y"], m["gy"], br.fold(br.draw_params(layer, block, 2)), s, Kc=f["wg1.Kc"])
    dz = np.where(m["y"] > 0, m["gy"], 0.0).astype(np.float64).reshape(-1, cout)
    x2 = br.patches(m["mid"], 1).reshape(dz.shape[0], -1)
    assert dz.shape[0] == f["wg1.npix"] and _runs(dz.shape[0], f["wg1.Kc"])[-1][1] == f["wg1.last"]
    assert _worst(br._torch_w(dz.T @ x2, cout, 9), R["dW2"], E["dW2"]) <= 1.0
    drop, twice = (br._torch_w(v, cout, 9) for v in _wgrad_mutants(dz, x2, f["wg1.Kc"]))
    _report(f"S block layer{layer}.{block} dW2'", {"last chunk dropped": _worst(drop, R["dW2"], E["dW2"]),
                                                   "first offset twice": _worst(twice, R["dW2"], E["dW2"])})


def test_split_k_and_second_pass_mutants_of_the_stem(dump):
    Wf = sr.fold(sr.draw_params(3))[0]
    c = next(c for c in gc.CASES if c.op == "stem" and "S" in c.regimes)
    f = _fields(dump, c)
    m = sr.draw_case(*c.shape, 5)
    R, E = sr.backward(m["x"], m["a"], m["gp"], Wf, Kc=f["wg.Kc"])
    d2, x2 = R["dA"].reshape(-1, 64), sr.patches(m["x"]).reshape(-1, 147)
    assert d2.shape[0] == f["wg.npix"] and _runs(d2.shape[0], f["wg.Kc"])[-1][1] == f["wg.last"]
    drop, twice = (v.reshape(64, 3, 7, 7) for v in _wgrad_mutants(d2, x2, f["wg.Kc"]))
    _report("S stem dW'", {"last chunk dropped": _worst(drop, R["dW"], E["dW"]),
                           "first offset twice": _worst(twice, R["dW"], E["dW"])})


def test_second_pass_mutants_of_the_stem_data_gradient(dump):
    Wf = sr.fold(sr.draw_params(3))[0]
    c = next(c for c in gc.CASES if c.op == "stem" and "G" in c.regimes)
    f = _fields(dump, c)
    B, H, W = c.shape
    m = sr.draw_case(B, H, W, 6)
    # dx and its bound alone: backward()'s expressions for them (the weight gradient plays no part here)
    dap, dabs = sr.pool_adjoint(m["a"], m["gp"])
    da, Eda = np.where(m["a"] > 0, dap, 0.0), np.where(m["a"] > 0, 3 * br.U24 * dabs, 0.0)
    aW = np.abs(np.asarray(Wf, np.float64))
    dx = sr.dgrad7(da, Wf, H, W)
    bound = br.U24 * np.abs(dx) + sr.DX_TERMS * br.U53 * sr.dgrad7(np.abs(da) + Eda, aW, H, W) + sr.dgrad7(Eda, aW, H, W)
    first = f["dg.blocks"] * f["dg.pixels"]  # the first pixel of a second pass
    assert f["npix_x"] == B * H * W and first < f["npix_x"]
    pix = dx.transpose(0, 2, 3, 1).reshape(-1, 3)  # pixel-major, as the kernel numbers them
    back = lambda v: v.reshape(B, H, W, 3).transpose(0, 3, 1, 2)  # noqa: E731
    unwritten, stale = pix.copy(), pix.copy()
    unwritten[first:] = 0.0
    stale[first:] = pix[:f["npix_x"] - first]
    _report("G stem dx", {"second passes unwritten": _worst(back(unwritten), dx, bound),
                          "second passes hold the first's": _worst(back(stale), dx, bound)})


@pytest.mark.parametrize("regime", ["Ps", "Pf"])
def test_partial_block_mutants_of_a_bias_gradient(dump, regime):
    c = next(c for c in gc.CASES if c.op == "block" and regime in c.regimes)
    f = _fields(dump, c)
    rng = np.random.default_rng(8)
    dz = br._half_zero(rng, (f["bs.npix"], f["bs.cout"])).astype(np.float64)
    r, e, _ = br._bgrad(dz, np.zeros_like(dz), False)  # backward()'s db2' of this dZ and its bound
    runs = _runs(f["bs.npix"], f["bs.pixels"])
    assert len(runs) == f["bs.blocks"] and runs[-1][1] == f["bs.last"]
    assert (regime == "Pf") == (f["bs.blocks"] == 256 and f["bs.last"] == f["bs.pixels"])
    _report(f"{regime} block db'", {"last block dropped": _worst(dz[:runs[-1][0]].sum(0), r, e)})
    # the batch statistics of block_train: the same blocks, S1 / n with the last block missing
    import block_train_restatement as tr
    z = rng.standard_normal((f["bs.npix"], f["bs.cout"])).astype(np.float32)
    (mean, _), (Em, _) = tr.stats_stage(z)
    _report(f"{regime} block_train mean", {"last block dropped": _worst(z[:runs[-1][0]].astype(np.float64).sum(0) / len(z), mean, Em)})


def test_partial_block_and_row_chunk_mutants_of_the_heads(dump):
    rng = np.random.default_rng(9)
    # Ph: db1 with the last hidden-gradient block dropped
    c = next(c for c in gc.CASES if c.op == "heads" and "Ph" in c.regimes)
    f = _fields(dump, c)
    n = c.shape[0] * c.shape[1] * c.shape[2]
    d = br._half_zero(rng, (n, 64)).astype(np.float64)
    ref, S = d.sum(0), np.abs(d).sum(0)
    kept = (f["dh_blocks"] - 1) * f["dh_pixels"]
    assert kept + f["dh_last"] == n
    _report("Ph heads db1", {"last block dropped": hr.worst_ratio(d[:kept].sum(0), ref, hr.bound_f64_sum(ref, S, n))})
    # R: the last chunk of frame 0 runs one row past the frame, into frame 1's first row
    c = next(c for c in gc.CASES if c.op == "heads" and "R" in c.regimes and c.args == (2,))
    f = _fields(dump, c)
    B, h, w = c.shape
    assert f["chunks_per_frame"] >= 2 and (f["chunks_per_frame"] - 1) * f["rows_per_chunk"] + f["last_rows"] == h
    C, O = 64, 64
    x = rng.standard_normal((B, h, w, C)).astype(np.float32)
    dA = br._half_zero(rng, (B, h, w, O))
    dW1, S1 = np.zeros((O, C, 3, 3)), np.zeros((O, C, 3, 3))
    extra = np.zeros((O, C, 3, 3))
    stack = np.zeros((B * h + 2, w + 2, C))  # the frames one below the other, as the flat row index sees them
    stack[1:B * h + 1, 1:w + 1] = x.reshape(B * h, w, C)
    d64 = dA.astype(np.float64)
    for ky, kx in hr.TAPS:
        xs = hr.shifted(x.astype(np.float64), ky, kx).reshape(-1, C)
        dW1[:, :, ky, kx] = d64.reshape(-1, O).T @ xs
        S1[:, :, ky, kx] = np.abs(d64).reshape(-1, O).T @ np.abs(xs)
        extra[:, :, ky, kx] = d64[1, 0].T @ stack[h + ky, kx:kx + w]  # row h of frame 0 = row 0 of frame 1
    bound = hr.bound_dW1(dW1, S1, f["Kc"], B * h * w)
    _report("R heads dW1", {"a chunk crosses the frame by one row": hr.worst_ratio(dW1 + extra, dW1, bound)})
