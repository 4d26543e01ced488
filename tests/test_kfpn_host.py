"""apply_kfpn as an operator on the host (no GPU): the restatement (tests/kfpn_restatement.py) against the
reference's apply_kfpn and autograd (tests/golden/gen_kfpn_golden.py) and against a finite difference of its own
forward; the two entry points' argument checks; the drop-in's apply_kfpn refuses CPU tensors.

Cases of the fixture: generic (B 2, heads 3/2/2/1/3, 8 x 12, level 0 at 4 x 6); fullres (the same shapes, level 0
at 8 x 12); saturated (levels 100 apart: the lowest level's weight is exactly 0 and the top one's exactly 1, the
middle one's is a float32 subnormal, e^-100); equal (the three levels bit-equal: weights 1/3); cancel (every other
element has 1 + v0 - out within float32 rounding of 0); tiny (B 1, one channel, 2 x 2 over 1 x 1); narrow (w = 6:
the scalar kernels, level-0 rows of 3 cells); onehead (num_heads = 1, 3 channels)."""
import ctypes

import numpy as np
import pytest

import golden_io
import kfpn_restatement as kr
from conftest import GOLDEN
from sfa_hip import _lib

CASES = ("generic", "fullres", "saturated", "equal", "cancel", "tiny", "narrow", "onehead")


@pytest.fixture(scope="module")
def g():
    return golden_io.load(GOLDEN, "kfpn_golden")


def case_inputs(g, name):
    """(heads, half, levels by head, upstream gradient by head) of one case."""
    heads = [str(n) for n in g[f"{name}/heads"]]
    levels = {h: [g[f"{name}/L/{h}/{l}"] for l in range(3)] for h in heads}
    return heads, bool(g[f"{name}/half"]), levels, {h: g[f"{name}/g/{h}"] for h in heads}


def zero_weight_masks(g, name, head, half):
    """Per level, where the reference's float32 weight is exactly 0 (for a half-resolution level 0: in all four
    children): the gradient there is exactly 0."""
    w = g[f"{name}/weights/{head}"] == 0
    m0 = w[..., 0]
    if half:
        m0 = m0[:, :, 0::2, 0::2] & m0[:, :, 0::2, 1::2] & m0[:, :, 1::2, 0::2] & m0[:, :, 1::2, 1::2]
    return [m0, w[..., 1], w[..., 2]]


def test_fixture_covers_the_cases(g):
    assert [str(n) for n in g["cases"]] == list(CASES)
    heads, half, lv, _ = case_inputs(g, "generic")
    assert heads == ["hm_cen", "cen_offset", "direction", "z_coor", "dim"] and half
    assert [lv[h][1].shape for h in heads] == [(2, c, 8, 12) for c in (3, 2, 2, 1, 3)]
    assert all(lv[h][0].shape == lv[h][1].shape[:2] + (4, 6) for h in heads)
    heads, half, lv, _ = case_inputs(g, "fullres")
    assert not half and all(lv[h][0].shape == lv[h][1].shape == (2, c, 8, 12) for h, c in zip(heads, (3, 2, 2, 1, 3)))
    heads, half, lv, _ = case_inputs(g, "saturated")
    for h in heads:
        v = np.stack([kr.upsample0(lv[h][0], half), lv[h][1], lv[h][2]], -1)
        gaps = np.diff(np.sort(v, axis=-1), axis=-1)
        assert np.all(np.abs(gaps - 100) < 3)
        w = np.sort(g[f"saturated/weights/{h}"], axis=-1)
        assert np.all(w[..., 0] == 0) and np.all(w[..., 2] == 1) and np.all(w[..., 1] < 1e-38)
    heads, half, lv, _ = case_inputs(g, "equal")
    for h in heads:
        assert not half and np.array_equal(lv[h][0], lv[h][1]) and np.array_equal(lv[h][0], lv[h][2])
        assert np.all(g[f"equal/weights/{h}"] == np.float32(1) / np.float32(3))
    heads, half, lv, _ = case_inputs(g, "cancel")
    for h in heads:
        out, _ = kr.forward64(lv[h], half)
        t = np.abs(1 + lv[h][0].astype(np.float64) - out)
        assert (t < 1e-6).sum() >= t.size // 2 and (t > 1e-2).any()
    heads, half, lv, _ = case_inputs(g, "tiny")
    assert half and heads == ["a"] and lv["a"][0].shape == (1, 1, 1, 1) and lv["a"][1].shape == (1, 1, 2, 2)
    heads, half, lv, _ = case_inputs(g, "narrow")
    assert half and lv[heads[0]][1].shape[3] == 6 and lv[heads[0]][0].shape[3] == 3 and len(heads) == 2
    heads, half, lv, _ = case_inputs(g, "onehead")
    assert half and len(heads) == 1 and lv[heads[0]][1].shape[1] == 3


@pytest.mark.parametrize("name", CASES)
def test_restatement_forward_matches_the_reference(g, name):
    """The project's per-kernel gate, <= 1e-5 max(1, |ref|) per element, for out and for the weights."""
    heads, half, lv, _ = case_inputs(g, name)
    for h in heads:
        out, wts = kr.forward(lv[h], half)
        for what, mine, ref in (("out", out, g[f"{name}/out/{h}"]), ("weights", wts, g[f"{name}/weights/{h}"])):
            assert mine.shape == ref.shape and mine.dtype == ref.dtype == np.float32
            err = np.abs(mine.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
            print(f"kfpn[{name}/{h}] {what}: max gated error {err.max():.3e}")
            assert err.max() <= kr.GATE, (name, h, what, err.max())


@pytest.mark.parametrize("name", CASES)
def test_restatement_gradient_matches_the_reference(g, name):
    """Every element of every level of every head within the gate; the recorded d_ref is what the test sees."""
    heads, half, lv, up = case_inputs(g, name)
    d_ref = np.zeros(3)
    for h in heads:
        mine = kr.grad(lv[h], up[h], half)
        masks = zero_weight_masks(g, name, h, half)
        for l in range(3):
            ref = g[f"{name}/grad/{h}/{l}"]
            assert mine[l].shape == ref.shape == lv[h][l].shape
            err = np.abs(mine[l] - ref) / np.maximum(1.0, np.abs(ref))
            assert err.max() <= kr.GATE, (name, h, l, err.max())
            d_ref[l] = max(d_ref[l], np.abs(mine[l] - ref).max())
            if name == "saturated":  # exact zeros, after the one rounding to float32
                assert masks[l].any() and np.all(ref[masks[l]] == 0) and np.all(mine[l].astype(np.float32)[masks[l]] == 0)
                assert np.array_equal(ref == 0, mine[l].astype(np.float32) == 0)
    print(f"kfpn[{name}] gradient: d_ref per level {d_ref}")
    np.testing.assert_array_equal(d_ref, g[f"{name}/d_ref"])


def test_gradient_equals_a_finite_difference_of_the_forward(g):
    """generic, float64: central differences of total = sum(out * g) over forward64, one level element at a time.
    With e the float64 epsilon the step is h = e^(1/3).  Bound per element: truncation h^2 |f'''| / 6 with
    |f'''| <= 16 (1 + V) sum_children |g|: for f = out as a function of v_j, f' = w_j t with t = 1 + v_j - f,
    f'' = w_j' t + w_j (1 - f'), f''' = w_j'' t + 2 w_j' (1 - f') - w_j f'', and |w_j'| <= 1/4, |w_j''| <= 1/10,
    |t| <= 1 + 2 V give |f'''| <= 4 (1 + V); the factor 4 above that is margin.  Plus the rounding of the two
    forward sums, 8 e sum|out * g| / h."""
    heads, half, lv, up = case_inputs(g, "generic")
    e = np.finfo(np.float64).eps
    step = e ** (1 / 3)
    checked = 0
    for h in heads:
        levels = [v.astype(np.float64) for v in lv[h]]
        gu = up[h].astype(np.float64)
        mine = kr.grad(levels, gu, half)
        absolute = kr.grad_bound(levels, gu, half)
        lsum = float(np.abs(kr.forward64(levels, half)[0] * gu).sum())
        for l in range(3):
            flat, got = levels[l].reshape(-1), mine[l].reshape(-1)
            # sum_children |g| (1 + V), from the restatement's own bound
            scale = ((absolute[l] - kr.GRAD_FLOOR) / kr.GRAD_ABS).reshape(-1)
            for i in range(flat.size):
                x = flat[i]
                flat[i] = x + step
                hi = float((kr.forward64(levels, half)[0] * gu).sum())
                flat[i] = x - step
                lo = float((kr.forward64(levels, half)[0] * gu).sum())
                flat[i] = x
                fd = (hi - lo) / ((x + step) - (x - step))
                bound = step ** 2 * 16 * scale[i] / 6 + 8 * e * lsum / step
                assert abs(fd - got[i]) <= bound, (h, l, i, fd, got[i], bound)
                checked += abs(got[i]) > 100 * bound
    assert checked > 500  # not vacuous: most elements are far above their bound


def _p(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def test_argument_errors_before_any_launch():
    """SFA_E_INVALID on the host, never touching the device; the message names the argument."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = _p(buf).value
    vp = ctypes.c_void_p

    def ptrs(n, spec):
        """spec: "ok" = n valid pointers, None = a NULL array, an index = that entry NULL."""
        if spec is None:
            return None
        a = (vp * n)(*[p] * n)
        if spec != "ok":
            a[spec] = None
        return a

    def chans(ch):
        return None if ch is None else (ctypes.c_int * 8)(*(list(ch) + [1] * (8 - len(ch))))

    def fwd(n=2, ch=(3, 2), B=2, h=8, w=12, half=1, levels="ok", out="ok", weights="ok"):
        m = n if 0 < n <= 8 else 1
        return L.sfa_kfpn_combine(ptrs(3 * m, levels), chans(ch), n, B, h, w, half, ptrs(m, out), ptrs(m, weights), None)

    def bwd(n=2, ch=(3, 2), B=2, h=8, w=12, half=1, levels="ok", grad_out="ok", grad_levels="ok"):
        m = n if 0 < n <= 8 else 1
        return L.sfa_kfpn_combine_grad(ptrs(3 * m, levels), chans(ch), n, B, h, w, half, ptrs(m, grad_out),
                                       ptrs(3 * m, grad_levels), None)

    shared = [({"levels": None}, b"null levels"), ({"ch": None}, b"null channels"), ({"levels": 4}, b"levels[4]"),
              ({"n": 0}, b"num_heads"), ({"n": 9}, b"num_heads"), ({"n": -1}, b"num_heads"),
              ({"B": 0}, b"B "), ({"B": 65536}, b"B "), ({"h": 0}, b"h "), ({"w": -4}, b"w "),
              ({"ch": (3, 0)}, b"channels[1]"), ({"ch": (65535, 1)}, b"channels sum"),
              ({"h": 7}, b"even h and w"), ({"w": 11}, b"even h and w"), ({"half": 2}, b"level0_half"),
              ({"h": 1 << 16, "w": 1 << 16}, b"h x w")]
    for call, who, own in ((fwd, b"kfpn_combine:", [({"out": None}, b"null out"), ({"out": 1}, b"out[1]"),
                                                  ({"weights": 0}, b"weights[0]")]),
                           (bwd, b"kfpn_combine_grad:", [({"grad_out": None}, b"null grad_out"),
                                                       ({"grad_levels": None}, b"null grad_levels"),
                                                       ({"grad_out": 1}, b"grad_out[1]"),
                                                       ({"grad_levels": 5}, b"grad_levels[5]")])):
        for kw, word in shared + own:
            assert call(**kw) == -1, (who, kw)
            msg = L.sfa_last_error_string()
            assert who in msg and word in msg, (kw, msg)


def test_abi_version_unchanged_and_symbols_present():
    import os
    import re
    from conftest import REPO
    assert _lib.lib().sfa_abi_version() == 2 == _lib.ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sfa_hip.h")).read(), flags=re.S)
    for sym in ("sfa_kfpn_combine", "sfa_kfpn_combine_grad"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), sym)
        assert re.search(r"\b%s\s*\(" % sym, header)


def test_cpu_tensors_are_refused():
    import torch
    from models import fpn_resnet, resnet
    from sfa_hip import runtime
    lv = [torch.zeros(1, 2, 4, 4) for _ in range(3)]
    model = fpn_resnet.get_pose_net(18, {"hm_cen": 3}, 64, False)
    with pytest.raises(_lib.SfaNativeError, match="GPU"):
        model.apply_kfpn(lv)
    for fn in (runtime.kfpn_combine, runtime.kfpn_heads):
        with pytest.raises(_lib.SfaNativeError, match="GPU"):
            fn({"a": lv})
    with pytest.raises(_lib.SfaNativeError, match="GPU"):
        runtime.kfpn_combine_grad({"a": lv}, {"a": lv[0]})
    # the plain resnet has no KFPN
    with pytest.raises(AttributeError):
        resnet.get_pose_net(18, {"hm_cen": 3}, 64, False).apply_kfpn(lv)
