"""PoseResNet.block_from_input, layers_from_pooled and detect_from_pooled on the GPU: backward is the C entries plus
the BatchNorm unfold bit for bit, .grad lands on x and every block parameter, the chain reaches 123 of the model's 126
parameters through the differentiable Compute_Loss, an in-place weight change is seen by the next call, the two
blocks of a layer against the model's own forward, and the plain resnet_18 refuses all of it."""
import numpy as np
import pytest
import torch

import block_restatement as br
import stage_cases as sc
from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu


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
    for L in (1, 2, 3, 4):
        for b in (0, 1):
            sd = br.state_entries(L, b, br.draw_params(L, b, 300 + 10 * L + b))
            own = dict(m.named_parameters())
            own.update(dict(m.named_buffers()))
            for k, v in sd.items():
                own[k].data.copy_(torch.from_numpy(v))
    return m


@pytest.mark.parametrize("layer,block,shape", [(1, 0, (2, 3, 5)), (2, 0, (2, 4, 6)), (4, 1, (1, 2, 3))])
def test_block_from_input_is_the_entries(gpu, model, layer, block, shape):
    cin, cout, s, ds = br.block_shape(layer, block)
    for p in model.parameters():
        p.grad = None
    gen = torch.Generator().manual_seed(layer * 10 + block)
    B, h, w = shape
    x = torch.randn((B, cin, h, w), generator=gen).to(gpu).requires_grad_()
    y = model.block_from_input(layer, block, x * 2)
    assert tuple(y.shape) == (B, cout, -(-h // s), -(-w // s)) and y.grad_fn is not None
    g = torch.randn(y.shape, generator=gen).to(gpu)
    (y * g).sum().backward()
    torch.cuda.synchronize()
    eng = model._engine(gpu)
    xn = (x.detach() * 2).permute(0, 2, 3, 1).contiguous()
    mid, yn = eng.block_forward(layer, block, xn)
    assert _bits(y.detach().permute(0, 2, 3, 1), yn)
    dx, dp = eng.block_grad(layer, block, xn, mid, yn, g.permute(0, 2, 3, 1).contiguous())
    assert x.grad is not None and _bits(x.grad, dx.permute(0, 3, 1, 2) * 2)
    mods = model._block_mods(layer, block)
    assert len(mods) == (3 if ds else 2)
    for i, (conv, bn) in enumerate(mods):
        dW, dg, dbt = runtime.bn_unfold_grad(conv.weight, bn.weight, bn.running_mean, bn.running_var, bn.eps,
                                             dp[(0, 2, 4)[i]], dp[(1, 3, 3)[i]])
        for p, d in ((conv.weight, dW), (bn.weight, dg), (bn.bias, dbt)):
            assert p.grad is not None and p.grad.shape == p.shape and _bits(p.grad, d)
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    # the unfolded gradients against the restatement's, at the bounds carried through the unfold
    pr = br.draw_params(layer, block, 300 + 10 * layer + block)
    f = br.fold(pr)
    c = dict(x=xn.cpu().numpy(), mid=mid.cpu().numpy(), y=yn.cpu().numpy(), gy=g.permute(0, 2, 3, 1).cpu().numpy())
    kc = eng.block_grad_chunk_pixels(layer, block, 0, B, h, w)
    R, E = br.backward(c["x"], c["mid"], c["y"], c["gy"], f, s, Kc=kc)
    for i, (ck, bk, (conv, bn)) in enumerate(zip(("conv1", "conv2", "convd"), ("bn1", "bn2", "bnd"), mods)):
        dwk, dbk = ("dW1", "dW2", "dWd")[i], ("db1", "db2", "db2")[i]
        (rW, rg, rb), (eW, eg, eb) = br.bn_unfold(pr[ck], pr[bk], R[dwk], R[dbk], E[dwk], E[dbk])
        for got, r, e in ((conv.weight.grad, rW, eW), (bn.weight.grad, rg, eg), (bn.bias.grad, rb, eb)):
            err = np.abs(got.cpu().numpy().astype(np.float64) - r)
            assert (err <= e).all(), (layer, block, ck, float(np.max(err / np.maximum(e, 1e-300))))


def test_running_statistics_whatever_training_says(gpu, model):
    x = torch.randn((1, 64, 4, 4), generator=torch.Generator().manual_seed(1)).to(gpu)
    with torch.no_grad():
        a = model.block_from_input(1, 0, x)
        model.train()
        try:
            b = model.block_from_input(1, 0, x)
        finally:
            model.eval()
    assert _bits(a, b)


def test_detect_from_pooled_reaches_123_parameters(gpu, model):
    from losses.losses import Compute_Loss
    for p in model.parameters():
        p.grad = None
    B, h, w = 2, 16, 24
    x = torch.randn((B, 64, h, w), generator=torch.Generator().manual_seed(21)).to(gpu).requires_grad_()
    outs = model.detect_from_pooled(x)
    assert list(outs) == list(runtime.DEFAULT_HEADS)
    for n, c in runtime.DEFAULT_HEADS.items():
        assert outs[n].shape == (B, c, h, w) and outs[n].grad_fn is not None
    tb = runtime.TargetBuilder(gpu, hm_size=(h, w))
    labels, offsets = synthetic.synthetic_labels(B, seed=2)
    total, _ = Compute_Loss(gpu, differentiable=True)(dict(outs), tb(labels, offsets))
    total.backward()
    torch.cuda.synchronize()
    assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    named = dict(model.named_parameters())
    assert len(named) == 126
    stem = {"conv1.weight", "bn1.weight", "bn1.bias"}
    reached = {k for k, p in named.items() if p.grad is not None}
    assert reached == set(named) - stem and len(reached) == 123
    for k in reached:
        assert torch.isfinite(named[k].grad).all() and float(named[k].grad.abs().max()) > 0, k
    bp = model.block_parameters()
    assert len(bp) == 57 and len({id(p) for p in bp}) == 57 and all(p.grad is not None for p in bp)
    ids = {id(p) for p in bp} | {id(p) for p in model.neck_parameters() + model.head_parameters()}
    assert len(ids) == 123


def test_in_place_weight_change_is_seen(gpu, model):
    layer, block, s = 2, 0, 2
    pr = br.draw_params(layer, block, 300 + 10 * layer + block)
    x = torch.randn((1, 64, 4, 6), generator=torch.Generator().manual_seed(5)).to(gpu)
    conv = model.layer2[0].conv1
    try:
        with torch.no_grad():
            before = model.block_from_input(layer, block, x)
            conv.weight.mul_(0.5)
            after = model.block_from_input(layer, block, x)
        assert not _bits(before, after)
        pr2 = dict(pr, conv1=(pr["conv1"] * np.float32(0.5)))
        xn = x.permute(0, 2, 3, 1).cpu().numpy()
        for got, p in ((before, pr), (after, pr2)):
            _, ry = br.forward(xn, br.fold(p), s)
            g = got.permute(0, 2, 3, 1).cpu().numpy()
            # two stages: the gate on mid carried through conv2 by its |W'| sums, plus the gate on y itself
            f = br.fold(p)
            rm, _ = br.forward(xn, f, s)
            carried = br.conv3(sc.GATE * np.maximum(1.0, np.abs(rm)), np.abs(f["W2"]), 1)
            assert (np.abs(g - ry) <= carried + sc.GATE * np.maximum(1.0, np.abs(ry))).all()
    finally:
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(pr["conv1"]))


@pytest.mark.parametrize("L", [2, 3, 4])
def test_two_blocks_against_the_models_forward(gpu, model, L):
    """layer{L}.0 then layer{L}.1 on the model's own LAYER{L-1} view against its LAYER{L} view: four convolution
    stages, each at the per-stage gate 1e-5 max(1, |v|), the gate of every stage carried through the convolutions
    after it by their |W'| sums (the ReLUs and the skips are 1-Lipschitz)."""
    B, H, W = 2, 64, 96
    eng = model._engine(gpu)
    xin = torch.from_numpy(synthetic.synthetic_bev(B, H, W, seed=4)).to(gpu)
    ws = torch.empty(eng.workspace_bytes(B, H, W), dtype=torch.uint8, device=gpu)
    eng.forward_into(xin, eng.alloc_outputs(B, H, W), _lib.IN_NCHW3, ws)
    views = eng.debug_views(ws, B, H, W)
    src, ref = views[f"layer{L - 1}"].clone(), views[f"layer{L}"].permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)
    with torch.no_grad():
        y0 = model.block_from_input(L, 0, src)
        y1 = model.block_from_input(L, 1, y0)
    torch.cuda.synchronize()
    got = y1.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)
    f0 = br.fold(br.draw_params(L, 0, 300 + 10 * L))
    f1 = br.fold(br.draw_params(L, 1, 300 + 10 * L + 1))
    xn = src.permute(0, 2, 3, 1).cpu().numpy()
    m0, o0 = br.forward(xn, f0, 2)
    m1, o1 = br.forward(o0, f1, 1)
    gate = lambda v: sc.GATE * np.maximum(1.0, np.abs(v))  # noqa: E731
    e = gate(m0)
    e = br.conv3(e, np.abs(f0["W2"]), 1) + gate(o0)
    e = br.conv3(br.conv3(e, np.abs(f1["W1"]), 1) + gate(m1), np.abs(f1["W2"]), 1) + e + gate(o1)
    # both sides are within e of the restatement
    q = float(np.max(np.abs(got - ref) / (2 * e)))
    print(f"layer{L}: blocks against the model's forward, difference / bound {q:.4f}")
    assert q <= 1.0


def test_plain_resnet_refuses(gpu):
    from models import resnet
    plain = resnet.get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False)
    x = torch.zeros((1, 64, 4, 4), device=gpu)
    for call in (plain.block_parameters, lambda: plain.block_from_input(1, 0, x), lambda: plain.layers_from_pooled(x),
                 lambda: plain.detect_from_pooled(x)):
        with pytest.raises(AttributeError):
            call()
