"""PoseResNet.heads_from_levels / level_heads on the GPU: the heads as an autograd operator over a caller's three level
inputs.  The operator is sfa_model_heads_forward, sfa_kfpn_combine and, in backward, sfa_kfpn_combine_grad,
sfa_model_heads_grad and sfa_model_heads_input_grad chained, so its results are compared bit for bit with direct calls
of those entries on the same inputs.  64 x 64 input geometry: levels 8 x 8, 16 x 16, 16 x 16; B 2."""
import pytest
import torch

from sfa_hip import _lib, runtime

pytestmark = pytest.mark.gpu

B = 2
SIZES = ((8, 8), (16, 16), (16, 16))


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def run(gpu):
    from models.fpn_resnet import get_pose_net
    torch.manual_seed(3)
    model = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False).to(gpu)
    gen = torch.Generator().manual_seed(5)
    for p in model.head_parameters():
        p.data = (torch.randn(p.shape, generator=gen) * (0.05 if p.dim() == 4 and p.shape[2] == 3 else 0.5)).to(gpu)
    frozen = [model.fpn1_dim[0].weight, model.fpn2_hm_cen[2].bias]
    for p in frozen:
        p.requires_grad_(False)
    leaves = [torch.randn((B, c, h, w), generator=gen).to(gpu).requires_grad_()
              for c, (h, w) in zip(_lib.HEADS_LEVEL_CIN, SIZES)]
    outs = model.heads_from_levels(*[t * 2 for t in leaves])
    g = {n: torch.randn(t.shape, generator=gen).to(gpu) for n, t in outs.items()}
    sum((outs[n] * g[n]).sum() for n in outs).backward()
    torch.cuda.synchronize()
    return model, leaves, outs, g, frozen


def test_operator_is_the_entries_chained(gpu, run):
    model, leaves, outs, g, frozen = run
    eng = model._engine(leaves[0].device)
    names = [n for n, _ in eng.heads]
    assert list(outs) == names and all(t.grad_fn is not None for t in outs.values())
    xs = [(t.detach() * 2).permute(0, 2, 3, 1).contiguous() for t in leaves]
    per_level = [eng.heads_forward(f, xs[f]) for f in range(3)]
    levels = {n: [lv[n] for lv in per_level] for n in names}
    direct = runtime.kfpn_combine(levels, level0_half=True)
    for n in names:
        assert outs[n].shape == (B, dict(eng.heads)[n], 16, 16) and _bits(outs[n].detach(), direct[n]), n
    glev = runtime.kfpn_combine_grad(levels, g, level0_half=True)
    params = model.head_parameters()
    for f in range(3):
        res, _, dA = eng.heads_param_grad(f, xs[f], {n: glev[n][f] for n in names}, want_hidden=True)
        dx = eng.heads_input_grad(f, dA).permute(0, 3, 1, 2)
        assert leaves[f].grad is not None and _bits(leaves[f].grad, dx * 2), f
        assert not torch.isnan(leaves[f].grad).any() and float(leaves[f].grad.abs().max()) > 0
        flat = [t for n in names for t in res[n]]
        for p, want in zip(params[20 * f:20 * f + 20], flat):
            if any(p is q for q in frozen):
                assert p.grad is None
            else:
                assert p.grad is not None and _bits(p.grad, want)
    assert sum(p.grad is not None for p in params) == 58


def test_heads_trainable_is_untouched(gpu, run):
    model = run[0]
    model.heads_trainable()
    try:
        for p in model.parameters():
            p.grad = None
        x = torch.randn((B, 3, 64, 64), generator=torch.Generator().manual_seed(9)).to(gpu).requires_grad_()
        out = model(x)
        sum(t.sum() for t in out.values()).backward()
        torch.cuda.synchronize()
        assert x.grad is None
        assert model.fpn0_hm_cen[0].weight.grad is not None and model.conv1.weight.grad is None
    finally:
        model.heads_trainable(False)
