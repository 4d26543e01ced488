"""PoseResNet.stem_from_image, detect_from_image and backbone_trainable() on the GPU: the stem operator under autograd
against the restatement (tests/stem_restatement.py), the whole chain from the image against the float64 restatement of
the network (tests/chain_restatement.py) at the gates tests/test_chain_host.py measured on the CPU, the trainable
mode's forward contract, and five steps of SGD over all 126 parameters."""
import numpy as np
import pytest
import torch

import chain_restatement as cr
import stem_restatement as sr
from sfa_hip import runtime
from test_chain_host import CASES, case_reference, model_state
from test_gpu_chain import _hold, _loss_backward, _param_grads, _zero

pytestmark = pytest.mark.gpu

# Learning rate of test_five_sgd_steps: plain SGD on the float64 restatement (chain_restatement.forward_backward from
# the fixture's image of c2_64x96, all 126 parameters updated) lowers the total loss on each of five steps at this rate,
# run on the CPU: 31.8870 -> 4.7972 -> 4.4293 -> 4.2429 -> 4.1161 -> 4.0189.  (1e-5 does too, more slowly: 31.8870 ->
# 13.1210 -> 10.2891 -> 8.8833 -> 8.0167 -> 7.4179; 1e-3 diverges on the first step, 31.9 -> 375.)
SGD_LR = 1e-4


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def model(gpu):
    from models.fpn_resnet import get_pose_net
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, False)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in model_state().items()})
    return m.to(gpu).eval()


def _stem_params(sd):
    return dict(conv1=sd["conv1.weight"], bn1=tuple(sd[f"bn1.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_stem_from_image_against_the_restatement(gpu, model):
    p = _stem_params(model_state())
    rng = np.random.default_rng(21)
    B, H, W = 2, 12, 20
    x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    _zero(model)
    xt = torch.from_numpy(x).to(gpu).requires_grad_()
    pooled = model.stem_from_image(xt)
    assert tuple(pooled.shape) == (B, 64, 3, 5)
    gp = rng.standard_normal((B, 3, 5, 64)).astype(np.float32)
    pooled.backward(torch.from_numpy(gp).to(gpu).permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    eng = model._engine(gpu)
    a, pn = eng.stem_forward(xt.detach())
    assert torch.equal(pn.permute(0, 3, 1, 2), pooled.detach())
    R, E = sr.unfolded(p, x, a.cpu().numpy(), gp, Kc=eng.stem_grad_chunk_pixels(B, H, W))
    got = {"dx": xt.grad, "conv1.weight": model.conv1.weight.grad, "bn1.weight": model.bn1.weight.grad,
           "bn1.bias": model.bn1.bias.grad}
    q = {k: sr.ratio(t.cpu().numpy(), R[k], E[k]) for k, t in got.items()}
    print("stem_from_image: error / bound " + " ".join(f"{k} {v:.4f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q
    assert [id(t) for t in model.stem_parameters()] == [id(model.conv1.weight), id(model.bn1.weight), id(model.bn1.bias)]


def test_stem_from_image_skips_what_needs_no_gradient(gpu, model, monkeypatch):
    eng = model._engine(gpu)
    seen = []
    real = eng.stem_grad
    monkeypatch.setattr(eng, "stem_grad", lambda *a, **kw: seen.append((kw["want_x"], tuple(kw["want_params"]))) or real(*a, **kw))
    x = torch.randn((1, 3, 8, 12), device=gpu)
    _zero(model)
    model.bn1.weight.requires_grad_(False)
    try:
        model.stem_from_image(x).sum().backward()
    finally:
        model.bn1.weight.requires_grad_(True)
    assert x.grad is None and seen == [(False, (True, True))]
    assert model.bn1.weight.grad is None and model.conv1.weight.grad is not None and model.bn1.bias.grad is not None
    _zero(model)
    model.conv1.weight.requires_grad_(False)
    model.bn1.weight.requires_grad_(False)
    try:
        xr = x.clone().requires_grad_()
        model.stem_from_image(xr).sum().backward()
    finally:
        model.conv1.weight.requires_grad_(True)
        model.bn1.weight.requires_grad_(True)
    assert xr.grad is not None and seen[-1] == (True, (False, True)) and model.conv1.weight.grad is None


@pytest.mark.parametrize("case", CASES)
def test_detect_from_image(gpu, model, case):
    r = case_reference(case)
    _zero(model)
    x = torch.from_numpy(r["inputs"]["image"]).to(gpu).requires_grad_()
    maps, loss = _loss_backward(gpu, case, model.detect_from_image(x))
    got = _param_grads(model, set(dict(model.named_parameters())))
    assert len(got) == 126
    got["x"] = x.grad.cpu().numpy()
    _hold(f"detect_from_image[{case}]", got, r["grads"], r["gate"])
    for h in cr.HEADS:
        m = cr.metric(maps[h], r["maps"][h]) / r["gate"][f"map/{h}"]
        print(f"  map {h}: m / gate {m.max():.3f}")
        assert np.all(m <= 1.0), h
    assert np.all(np.abs(loss - r["loss"]) <= 1e-3 * np.abs(r["loss"]))


def test_backbone_trainable_forward_contract(gpu, model):
    case = "c1_32x160"
    x = torch.from_numpy(case_reference(case)["inputs"]["image"]).to(gpu)
    plain = model(x)
    assert all(not t.requires_grad for t in plain.values())
    model.neck_trainable()
    model.backbone_trainable()
    try:
        outs = model(x)  # the deepest mode wins over neck_trainable
        ref = model.detect_from_image(x)
        assert list(outs) == list(ref) and all(_bits(outs[k], ref[k]) and outs[k].grad_fn is not None for k in ref)
        with torch.no_grad():
            quiet = model(x)
        assert all(_bits(quiet[k], plain[k]) and not quiet[k].requires_grad for k in plain)
        with pytest.raises(ValueError):
            model.forward_layout(x, runtime._lib.IN_NCHW3_FLIP_HW)
        # the operators' maps equal the fused forward within the composed forward gate, not bit for bit
        r = case_reference(case)
        for h in cr.HEADS:
            assert np.all(cr.metric(outs[h].detach().cpu().numpy(), r["maps"][h]) <= r["gate"][f"map/{h}"])
        # two backward passes without zeroing give exactly twice the first .grad
        _zero(model)
        _loss_backward(gpu, case, model(x))
        first = [p.grad.clone() for p in model.parameters()]
        _loss_backward(gpu, case, model(x))
        assert all(_bits(p.grad, 2 * f) for p, f in zip(model.parameters(), first))
    finally:
        model.backbone_trainable(False)
        model.neck_trainable(False)
    off = model(x)
    assert all(_bits(off[k], plain[k]) and off[k].grad_fn is None for k in plain)


def test_five_sgd_steps(gpu):
    from losses.losses import Compute_Loss
    from models.fpn_resnet import get_pose_net
    from test_gpu_chain import _targets
    case = "c2_64x96"
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, False)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in model_state().items()})
    m = m.to(gpu).eval().backbone_trainable()
    before = [p.detach().clone() for p in m.parameters()]
    assert len(before) == 126
    opt = torch.optim.SGD(m.parameters(), lr=SGD_LR)
    x = torch.from_numpy(case_reference(case)["inputs"]["image"]).to(gpu)
    tg = _targets(gpu, case)
    crit = Compute_Loss(gpu, differentiable=True)
    losses = []
    for _ in range(6):  # five updates, the loss read before each and after the last
        opt.zero_grad()
        total, _ = crit(dict(m(x)), tg)
        losses.append(float(total.detach()))
        if len(losses) <= 5:
            total.backward()
            opt.step()
    print("SGD losses " + " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < losses[0]
    assert all(not torch.equal(p.detach(), b) for p, b in zip(m.parameters(), before))
