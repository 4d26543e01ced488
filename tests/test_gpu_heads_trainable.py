"""PoseResNet.heads_trainable(): the forward's bits, the 60 .grad against the three gradient operators called by
hand, an upstream factor, requires_grad=False, and the repack after an optimiser step (64 x 64 input, B 2)."""
import numpy as np
import pytest
import torch

from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _model(gpu):
    from models.fpn_resnet import get_pose_net
    model = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False)
    sd = synthetic.synthetic_state_dict(_lib.state_layout(model._arch), 4)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    return model.to(gpu).eval()


def _targets(gpu, B, hm):
    tb = runtime.TargetBuilder(gpu, hm_size=(hm, hm))
    labels, offsets = synthetic.synthetic_labels(B, seed=2)
    return tb(labels, offsets)


def test_trainable_heads_plumbing(gpu):
    from losses.losses import Compute_Loss
    model = _model(gpu)
    B, H = 2, 64
    x = torch.from_numpy(synthetic.synthetic_bev(B, H, H, seed=3)).to(gpu)
    base = model(x)
    assert not any(t.requires_grad for t in base.values())
    model.heads_trainable()
    frozen = model.fpn1_dim[2].bias
    frozen.requires_grad_(False)
    outs = model(x)
    for k in base:
        assert outs[k].requires_grad and _bits(outs[k].detach(), base[k]), k  # the default forward's bits
    tg = _targets(gpu, B, H // 4)
    crit = Compute_Loss(gpu, differentiable=True)
    total, _ = crit(dict(outs), tg)
    total.backward()
    params = model.head_parameters()
    assert len(params) == 60
    assert frozen.grad is None and all(p.grad is not None for p in params if p is not frozen)

    # by hand: LossEvaluator.grad -> kfpn_combine_grad -> heads_param_grad on the same engine and a fresh forward
    eng = model._engine(x.device)
    ws = torch.empty(eng.workspace_bytes(B, H, H), dtype=torch.uint8, device=gpu)
    maps = eng.forward_into(x, eng.alloc_outputs(B, H, H), _lib.IN_NCHW3, ws)
    g = runtime.LossEvaluator(gpu).grad(maps, tg, apply_sigmoid=True)
    levels = {n: [t.contiguous() for t in lv] for n, lv in eng.debug_views(ws, B, H, H)["levels"].items()}
    glev = runtime.kfpn_combine_grad(levels, g, level0_half=True)
    want = []
    for level in range(3):
        res = eng.heads_param_grad(level, eng.level_input(ws, B, H, H, level), {n: glev[n][level] for n in levels})
        for n, _ in eng.heads:
            want += list(res[n])
    assert any(float(w.abs().max()) > 0 for w in want)
    # level_input on its own: the heads restated in float64 on it reproduce the level maps the forward left
    import heads_grad_restatement as hr
    for level in range(3):
        xin = eng.level_input(ws, B, H, H, level).cpu().numpy()
        for n, _ in eng.heads:
            seq = getattr(model, f"fpn{level}_{n}")
            prm = [t.detach().cpu().numpy() for t in (seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias)]
            worst, ok = hr.gate(levels[n][level].cpu().numpy(), hr.forward(xin, *prm)[2])
            assert ok, (level, n, worst)
    for p, w in zip(params, want):
        if p is not frozen:
            assert _bits(p.grad, w)

    # a 0.5 upstream factor halves every gradient exactly
    for p in params:
        p.grad = None
    total, _ = crit(dict(model(x)), tg)
    (total * 0.5).backward()
    for p, w in zip(params, want):
        if p is not frozen:
            assert _bits(p.grad, w * 0.5)

    # one SGD step on the head parameters: the engine repacks, the next forward differs
    opt = torch.optim.SGD([p for p in params if p.requires_grad], lr=0.1)
    opt.step()
    with torch.no_grad():
        after = model(x)
    assert not any(t.requires_grad for t in after.values())
    assert any(not _bits(after[k], base[k]) for k in base)
    # off again: today's path
    model.heads_trainable(False)
    assert not any(t.requires_grad for t in model(x).values())
