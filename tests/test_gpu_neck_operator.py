"""PoseResNet.neck_from_layers / detect_from_layers / neck_trainable on the GPU: the FPN neck as an autograd operator
and the neck-and-heads fine-tuning mode of the model's own forward.  Both are chains of C entries, so their results
are compared bit for bit with direct calls of those entries on the same inputs, at the two input sizes 160 x 160 and
192 x 192 (h4 = w4 = 5 and 6), B 2.  What ties the float32 neck to the model's own fused fp16x3 FPN stage, and checks
the workspace views neck_trainable() hands to sfa_model_neck_grad independently of that entry, is
test_detect_from_layers_against_the_models_forward at 160 x 192, whose bound is derived in its docstring."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_cases as gc
import neck_restatement as nr
import stage_cases as sc
from sfa_hip import _lib, runtime

pytestmark = pytest.mark.gpu

B, H, W = 2, 160, 192
H4, W4 = H // 32, W // 32
SIZES = [(160, 160), (192, 192)]


@pytest.fixture(autouse=True)
def _grad_mode():
    """Autograd on whatever an earlier test module left the process-wide switch at."""
    with torch.enable_grad():
        yield


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def model(gpu):
    from models.fpn_resnet import get_pose_net
    torch.manual_seed(3)
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False).to(gpu)
    gen = torch.Generator().manual_seed(5)
    for p in m.head_parameters():
        p.data = (torch.randn(p.shape, generator=gen) * (0.05 if p.dim() == 4 and p.shape[2] == 3 else 0.5)).to(gpu)
    for p in m.neck_parameters():
        p.data = (torch.randn(p.shape, generator=gen) * (p.shape[1] ** -0.5 if p.dim() == 4 else 1.0)).to(gpu)
    return m


def _layers(gpu, seed, grad=True, hw=(H, W)):
    gen = torch.Generator().manual_seed(seed)
    h4, w4 = hw[0] // 32, hw[1] // 32
    out = [torch.randn((B, c, h4 << (3 - i), w4 << (3 - i)), generator=gen).to(gpu) for i, c in enumerate(_lib.NECK_LAYER_C)]
    return [t.requires_grad_() for t in out] if grad else out


@pytest.mark.parametrize("hw", SIZES)
def test_neck_from_layers_is_the_entries(gpu, model, hw):
    H4, W4 = hw[0] // 32, hw[1] // 32
    frozen = model.conv_up_level2.bias
    frozen.requires_grad_(False)
    try:
        for p in model.parameters():
            p.grad = None
        leaves = _layers(gpu, 7, hw=hw)
        us = model.neck_from_layers(*[t * 2 for t in leaves])
        assert [tuple(t.shape) for t in us] == [(B, 256, 4 * H4, 4 * W4), (B, 128, 8 * H4, 8 * W4), (B, 64, 8 * H4, 8 * W4)]
        assert all(t.grad_fn is not None for t in us)
        gen = torch.Generator().manual_seed(8)
        gs = [torch.randn(t.shape, generator=gen).to(gpu) for t in us]
        sum((u * g).sum() for u, g in zip(us, gs)).backward()
        torch.cuda.synchronize()
        eng = model._engine(gpu)
        ls = [(t.detach() * 2).permute(0, 2, 3, 1).contiguous() for t in leaves]
        du = eng.neck_forward(*ls)
        for a, b in zip(us, du):
            assert _bits(a.detach().permute(0, 2, 3, 1), b)
        dl, dp = eng.neck_grad(*[g.permute(0, 2, 3, 1).contiguous() for g in gs], layers=ls, ups=du[:2])
        for leaf, d in zip(leaves, dl):
            assert leaf.grad is not None and _bits(leaf.grad, d.permute(0, 3, 1, 2) * 2)
            assert torch.isfinite(leaf.grad).all() and float(leaf.grad.abs().max()) > 0
        for p, d in zip(model.neck_parameters(), dp):
            if p is frozen:
                assert p.grad is None
            else:
                assert p.grad is not None and _bits(p.grad, d)
    finally:
        frozen.requires_grad_(True)


def test_detect_from_layers_reaches_all_66_parameters(gpu, model):
    for p in model.parameters():
        p.grad = None
    leaves = _layers(gpu, 11)
    outs = model.detect_from_layers(*leaves)
    assert list(outs) == list(runtime.DEFAULT_HEADS)
    for n, c in runtime.DEFAULT_HEADS.items():
        assert outs[n].shape == (B, c, 8 * H4, 8 * W4) and outs[n].grad_fn is not None
    sum(t.sum() for t in outs.values()).backward()
    torch.cuda.synchronize()
    got = model.neck_parameters() + model.head_parameters()
    assert len(got) == 66 and all(p.grad is not None and torch.isfinite(p.grad).all() for p in got)
    assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in leaves)
    assert model.conv1.weight.grad is None
    # the same maps as the two operators chained by hand
    with torch.no_grad():
        again = model.heads_from_levels(*model.neck_from_layers(*[t.detach() for t in leaves]))
    for n in outs:
        assert _bits(outs[n].detach(), again[n])


@pytest.mark.parametrize("hw", SIZES)
def test_neck_trainable(gpu, model, hw):
    H, W = hw
    x = torch.randn((B, 3, H, W), generator=torch.Generator().manual_seed(9)).to(gpu).requires_grad_()
    with torch.no_grad():
        plain = model(x)
    assert all(t.grad_fn is None for t in plain.values())
    gen = torch.Generator().manual_seed(10)
    g = {n: torch.randn(t.shape, generator=gen).to(gpu) for n, t in plain.items()}

    def grads(mode):
        for p in model.parameters():
            p.grad = None
        getattr(model, mode)()
        try:
            out = model(x)
            sum((out[n] * g[n]).sum() for n in out).backward()
            torch.cuda.synchronize()
        finally:
            getattr(model, mode)(False)
        return out, [None if p.grad is None else p.grad.clone() for p in model.neck_parameters() + model.head_parameters()]

    out, got = grads("neck_trainable")
    for n in plain:
        assert out[n].grad_fn is not None and _bits(out[n].detach(), plain[n]), n
    assert x.grad is None and model.conv1.weight.grad is None and model.layer4[1].conv2.weight.grad is None
    assert all(t is not None and torch.isfinite(t).all() for t in got)
    _, heads_only = grads("heads_trainable")
    assert all(t is None for t in heads_only[:6])
    for a, b in zip(got[6:], heads_only[6:]):
        assert _bits(a, b)  # the 60 head gradients are heads_trainable()'s
    # the direct chain of entries on the workspace views of one more forward
    eng = model._engine(gpu)
    ws = torch.empty(eng.workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)
    eng.forward_into(x.detach(), eng.alloc_outputs(B, H, W), _lib.IN_NCHW3, ws)
    views = eng.debug_views(ws, B, H, W)
    levels = {n: [t.contiguous() for t in lv] for n, lv in views["levels"].items()}
    glev = runtime.kfpn_combine_grad(levels, g, level0_half=True)
    gx = []
    for level in range(3):
        _, _, dA = eng.heads_param_grad(level, eng.level_input(ws, B, H, W, level),
                                        {n: glev[n][level] for n, _ in eng.heads}, want_hidden=True)
        gx.append(eng.heads_input_grad(level, dA))
    nhwc = lambda k: views[k].permute(0, 2, 3, 1)  # noqa: E731
    _, dp = eng.neck_grad(*gx, layers=[nhwc(f"layer{i}") for i in (1, 2, 3, 4)], ups=[nhwc("up_level2"), nhwc("up_level3")],
                          want_layers=(False,) * 4)
    torch.cuda.synchronize()
    for a, b in zip(got[:6], dp):
        assert _bits(a, b)
    # an SGD step moves conv_up_level1.weight and the next forward uses it; with the mode off nothing carries a grad_fn
    with torch.no_grad():
        before = model.conv_up_level1.weight.clone()
        model.conv_up_level1.weight -= 0.05 * got[0]
        assert not torch.equal(before, model.conv_up_level1.weight)
        moved = model(x)
        assert any(not _bits(moved[n], plain[n]) for n in plain)
        model.conv_up_level1.weight.copy_(before)
        back = model(x)
    assert all(_bits(back[n], plain[n]) for n in plain)
    assert all(t.grad_fn is None for t in model(x).values())


def test_refusals(gpu, model):
    from models import resnet
    eng = model._engine(gpu)
    big = eng.max_batch(H, W) + 1
    model.neck_trainable()
    try:
        with pytest.raises(ValueError):
            model(torch.empty((big, 3, H, W), device=gpu))
    finally:
        model.neck_trainable(False)
    with pytest.raises(ValueError):
        model.neck_from_layers(*_layers(gpu, 1, grad=False)[::-1])
    plain = resnet.get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False)
    for call in (plain.neck_trainable, plain.neck_parameters, lambda: plain.neck_from_layers(None, None, None, None)):
        with pytest.raises(AttributeError):
            call()


# ----------------------------------------------------------------- the operator against the model's own forward
GATE = sc.GATE * (1 + 2e-5)  # the per-kernel gate, taken on the computed value instead of the exact one (below)


def _ideal_up_matrix(n):
    """U of one axis with exact coefficients: src = o (n - 1) / (2 n - 1) in float64 (what the float64 oracle
    stage of tests/stage_cases.py interpolates with, up to float64 rounding)."""
    M = np.zeros((2 * n, n))
    for o in range(2 * n):
        f = o * (n - 1) / (2 * n - 1) if n > 1 else 0.0
        i0 = min(int(np.floor(f)), n - 1)
        i1 = min(i0 + 1, n - 1)
        M[o, i0] += 1.0 - (f - i0)
        M[o, i1] += f - i0
    return M


def _coef_gap(xabs):
    """|U32 x - U64 x| <= (|dUy| (x) Ux32 + Uy64 (x) |dUx|) |x|: the resize with the kernels' float32 coefficients
    against the ideal one, elementwise, from the two matrices themselves."""
    h, w = xabs.shape[1:3]
    y32, x32, y64, x64 = nr.up_matrix(h), nr.up_matrix(w), _ideal_up_matrix(h), _ideal_up_matrix(w)
    e = lambda a, b: np.einsum("yh,xw,bhwc->byxc", a, b, xabs, optimize=True)  # noqa: E731
    return e(np.abs(y32 - y64), x32) + e(y64, np.abs(x32 - x64))


def _np(t):  # NCHW tensor -> NHWC float64
    return t.detach().permute(0, 2, 3, 1).contiguous().cpu().double().numpy()


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def golden_model(golden, gpu):
    """The model test_gpu_model_stages.py holds to the per-kernel gate (natural amplitudes), production kernels."""
    from models.fpn_resnet import get_pose_net
    m = get_pose_net(18, dict(gc.HEADS), 64, imagenet_pretrained=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gc.state_dict_np(golden.model).items()})
    return m.to(gpu).eval()


def test_detect_from_layers_against_the_models_forward(gpu, golden_model):
    """detect_from_layers fed the model's own layer1..4 workspace views (the views neck_trainable() hands to
    sfa_model_neck_grad) against the model's up_level2/3/4, per-level head maps and five outputs, sparse 2 x 160 x 192.

    Bound, every term an elementwise array.  G(v) = 1e-5 max(1, |v|) is the documented per-kernel gate of the model's
    stages against the float64 oracle stage on the stage's own inputs (tests/test_gpu_model_stages.py holds this
    model and this batch to it); it is taken on the computed value, max(1, |exact|) <= (1 + 2e-5) max(1, |computed|).
      neck.  D2 = |operator u2 - model up_level2| <= E2 + C + G: E2 neck_restatement's chained bound of the float32
        kernels against the restatement (U l4, convolution, U), C the gap between the restatement's float32 resize
        coefficients and the oracle's exact ones (_coef_gap, carried through the convolution like an input error), G
        the model's gate.  Stage 2 starts from two different inputs, the operator's u2 and the model's up_level2, at
        most D2 apart: the stage is linear, so D2 is carried through it as an input error (|W2a| D2, then U), and
        the stage's own E, C and G are added: D3; likewise D4.
      heads.  Y(x) = W2 ReLU(conv3x3(x; W1) + b1) + b2 is 1-Lipschitz through the ReLU: |Y(xo) - Y(xm)| <= |W2|
        conv3x3(D; |W1|).  The model's level map is within G of Y(xm).  The operator's Hd is within the same gate of
        the exact hidden activation (fp16x3 recompute, tests/test_gpu_heads_dgrad.py) and its y is that Hd through
        W2 in float64 rounded once (<= 2 u max(1, |y|) with the float64 sum): |W2| G(Hd) + 2 u max(1, |y|).
      combine.  f(v) = sum_j v_j softmax(v)_j has df/dv_j = s_j (1 + v_j - f), f lies between min v and max v, and
        moving every logit by at most d changes s_j by a factor of at most e^(2 d).  Along the segment between the
        model's level maps v and the operator's (|dv_j| <= Dy_j <= d): |f(vo) - f(vm)| <= e^(2 d) (1 + R + 2 d)
        sum_j s_j(vm) Dy_j with R = max v - min v.  Both combines are the same float32 kernel arithmetic, each within
        G of f: + 2 G.
    Carried through three stages of |W| sums the chained bound is wide behind the neck (the second printed line has
    the largest bound of each group), so the heads and the combine are also held stage by stage on identical inputs,
    where nothing is inherited: the operator's heads on the model's own up_level maps against the model's level maps
    (|W2| G(Hd) + 2 u max(1, |y|) + G), and sfa_kfpn_combine on the model's level maps against its outputs (2 G)."""
    model = golden_model
    eng = model._engine(gpu)
    x = torch.from_numpy(sc.sparse_batch(B, H, W, 71)).to(gpu)
    with torch.no_grad():
        ws = torch.empty(eng.workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)
        outs = eng.forward_into(x, eng.alloc_outputs(B, H, W), workspace=ws)
        torch.cuda.synchronize()
        views = eng.debug_views(ws, B, H, W)
        layers = [views[f"layer{i}"] for i in (1, 2, 3, 4)]
        us = model.neck_from_layers(*layers)
        got = model.detect_from_layers(*layers)
        per_level = [eng.heads_forward(f, us[f].permute(0, 2, 3, 1).contiguous(), want_hidden=True) for f in range(3)]
        same_in = [eng.heads_forward(f, eng.level_input(ws, B, H, W, f), want_hidden=True) for f in range(3)]
        levels_m = {n: [t.contiguous() for t in lv] for n, lv in views["levels"].items()}
        comb = runtime.kfpn_combine(levels_m, level0_half=True)
        torch.cuda.synchronize()
    u = 2.0 ** -24
    gate = lambda v: GATE * np.maximum(1.0, np.abs(v))  # noqa: E731
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    W1, b1, W2, b2, W3, b3 = [sd[f"conv_up_level{f}.{k}"].numpy().reshape(sd[f"conv_up_level{f}.{k}"].shape[0], -1).squeeze()
                              for f in (1, 2, 3) for k in ("weight", "bias")]
    l1, l2, l3, l4 = (_np(t) for t in layers)
    uo = [_np(t) for t in us]
    um = [_np(views[k]) for k in ("up_level2", "up_level3", "up_level4")]
    # neck: D2, D3, D4
    a, Ea = nr.up_b(l4)
    z, Ez = nr.conv(a, l3, W1, b1, Ea + _coef_gap(np.abs(l4)))
    _, E = nr.up_b(z, Ez)
    D = [E + _coef_gap(np.abs(z) + Ez) + gate(um[0])]
    z, Ez = nr.conv(uo[0], l2, W2, b2, D[0])
    _, E = nr.up_b(z, Ez)
    D.append(E + _coef_gap(np.abs(z) + Ez) + gate(um[1]))
    _, Ez = nr.conv(uo[1], l1, W3, b3, D[1])
    D.append(Ez + gate(um[2]))
    worst, widest = {}, {}
    for k, o, m, d in zip(("u2", "u3", "u4"), uo, um, D):
        assert o.shape == m.shape and np.isfinite(o).all()
        worst[k], widest[k] = float(np.max(np.abs(o - m) / d)), float(d.max())
    # heads and combine, per head
    up0 = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)  # noqa: E731
    for j, (n, c) in enumerate(eng.heads):
        vm, Dy = [], []
        for f in range(3):
            ys, hd = per_level[f]
            w1 = sd[f"fpn{f}_{n}.0.weight"].abs()
            w2 = sd[f"fpn{f}_{n}.2.weight"].abs().reshape(c, 64)
            lip = torch.einsum("co,bohw->bchw", w2, F.conv2d(_nchw(D[f]), w1, padding=1))
            hid = hd[..., 64 * j:64 * j + 64].cpu().double().permute(0, 3, 1, 2)
            own = torch.einsum("co,bohw->bchw", w2, GATE * hid.abs().clamp(min=1.0))
            yo, ym = ys[n].cpu().double(), views["levels"][n][f].cpu().double()
            d = lip + own + 2 * u * yo.abs().clamp(min=1.0) + GATE * ym.abs().clamp(min=1.0)
            worst[f"L{f}/{n}"] = float(((yo - ym).abs() / d).max())
            widest[f"L{f}"] = max(widest.get(f"L{f}", 0.0), float(d.max()))
            ys1, hd1 = same_in[f]
            hid1 = hd1[..., 64 * j:64 * j + 64].cpu().double().permute(0, 3, 1, 2)
            y1 = ys1[n].cpu().double()
            d1 = (torch.einsum("co,bohw->bchw", w2, GATE * hid1.abs().clamp(min=1.0)) + 2 * u * y1.abs().clamp(min=1.0)
                  + GATE * ym.abs().clamp(min=1.0))
            worst[f"same-input L{f}/{n}"] = float(((y1 - ym).abs() / d1).max())
            widest["same-input L"] = max(widest.get("same-input L", 0.0), float(d1.max()))
            vm.append(up0(ym) if f == 0 else ym)
            Dy.append(up0(d) if f == 0 else d)
        v, d3 = torch.stack(vm, -1), torch.stack(Dy, -1)
        s = torch.softmax(v, -1)
        dmax = d3.max(-1).values
        R = v.max(-1).values - v.min(-1).values
        om, oo = outs[n].cpu().double(), got[n].cpu().double()
        bound = torch.exp(2 * dmax) * (1 + R + 2 * dmax) * (s * d3).sum(-1) + GATE * (om.abs().clamp(min=1.0)
                                                                                       + oo.abs().clamp(min=1.0))
        assert oo.shape == om.shape and torch.isfinite(oo).all()
        worst[f"out/{n}"] = float(((oo - om).abs() / bound).max())
        widest["out"] = max(widest.get("out", 0.0), float(bound.max()))
        c1 = comb[n].cpu().double()
        worst[f"same-input out/{n}"] = float(((c1 - om).abs() / (GATE * (om.abs().clamp(min=1.0) + c1.abs().clamp(min=1.0)))).max())
    print("detect_from_layers vs the model's forward, difference / bound: "
          + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print("largest bound of an element: " + " ".join(f"{k} {v:.2e}" for k, v in widest.items()))
    assert max(worst.values()) <= 1.0, worst
