"""PoseResNet.stem_from_image / detect_from_image / backbone_trainable with ``batch_stats=True`` on the GPU: the engine
is not called, .grad lands on x and conv1.weight, bn1.weight, bn1.bias and equals the C entries bit for bit, bn1's
running buffers move as nn.BatchNorm2d moves them in train() (the fixture's within the carried bound) and stay with
``update_running=False``; the whole detector leaves a finite non-zero .grad at all 126 parameters and moves all 20
BatchNorms' buffers; backbone_trainable(batch_stats=True) is that call with grad on and today's fused forward under
no_grad; the defaults are bit-equal to calls without the new keywords; an optimiser step hands over to the engine."""
import os

import numpy as np
import pytest
import torch

import golden_io
import stem_train_restatement as st
from sfa_hip import runtime

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _fresh(gpu, seed=5):
    from models.fpn_resnet import get_pose_net
    torch.manual_seed(seed)
    return get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False).to(gpu)


@pytest.fixture(scope="module")
def model(gpu):
    return _fresh(gpu)


def _load_fixture(m, g):
    with torch.no_grad():
        m.conv1.weight.copy_(torch.from_numpy(g["conv1.weight"]))
        for t, k in ((m.bn1.weight, "weight"), (m.bn1.bias, "bias"), (m.bn1.running_mean, "running_mean"),
                     (m.bn1.running_var, "running_var")):
            t.copy_(torch.from_numpy(g[f"bn1.{k}"]))
        m.bn1.num_batches_tracked.zero_()


def _bn_state(m):
    return [(b.running_mean.clone(), b.running_var.clone(), int(b.num_batches_tracked))
            for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]


@pytest.mark.parametrize("name", ["b2_12x20", "b1_6x10"])
def test_stem_batch_stats_is_the_entries_and_moves_bn1(gpu, name, monkeypatch):
    g = golden_io.load(GOLDEN, "stem_train_golden")
    m = _fresh(gpu)
    _load_fixture(m, g)
    for p in m.parameters():
        p.grad = None
    monkeypatch.setattr(type(m), "_engine", lambda self, device: pytest.fail("batch_stats=True called the engine"))
    x = torch.from_numpy(g[f"{name}/x"]).to(gpu).requires_grad_()
    gp = torch.from_numpy(g[f"{name}/gp"]).to(gpu)  # NHWC
    pooled = m.stem_from_image(x, batch_stats=True)
    assert pooled.grad_fn is not None and tuple(pooled.shape) == (gp.shape[0], 64, gp.shape[1], gp.shape[2])
    (pooled * gp.permute(0, 3, 1, 2)).sum().backward()
    torch.cuda.synchronize()
    ps = [p.detach() for p in m.stem_parameters()]
    maps = runtime.stem_train_forward(x.detach(), ps, m.bn1.eps)
    assert _bits(pooled.detach().permute(0, 2, 3, 1), maps["pooled"])
    dx, dp = runtime.stem_train_grad(x.detach(), maps, gp, ps, m.bn1.eps)
    assert _bits(x.grad, dx)
    for p, d in zip(m.stem_parameters(), dp):
        assert p.grad is not None and _bits(p.grad, d) and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    # the running buffers after the step against the fixture's, within the carried bound of both
    p = dict(conv1=g["conv1.weight"], bn1=tuple(g[f"bn1.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))
    xs = g[f"{name}/x"]
    V, E = st.forward_chain(xs, p)
    _, E32 = st.forward_chain(xs, p, f32=True)
    n = int(np.prod(maps["z"].shape[:3]))
    assert int(m.bn1.num_batches_tracked) == int(g[f"{name}/num_batches_tracked"]) == 1
    for which, (buf, key) in enumerate(((m.bn1.running_mean, "running_mean"), (m.bn1.running_var, "running_var"))):
        before = p["bn1"][2 + which]
        bound = (st.running_bound(before, V["stats"][which], E["stats"][which], n, which)
                 + st.running_bound(before, V["stats"][which], E32["stats"][which], n, which))
        q = st.ratio(buf.cpu().numpy(), g[f"{name}/{key}_after"].astype(np.float64), bound)
        print(name, key, "error / bound", q)
        assert q <= 1.0
        assert st.ratio(buf.cpu().numpy(), st.running_update(before, V["stats"][which], n, which),
                        st.running_bound(before, V["stats"][which], E["stats"][which], n, which)) <= 1.0
    # update_running=False leaves them bit-untouched
    now = _bn_state(m)
    with torch.no_grad():
        again = m.stem_from_image(x.detach(), batch_stats=True, update_running=False)
    assert _bits(again, pooled.detach())
    assert all(_bits(a[0], b[0]) and _bits(a[1], b[1]) and a[2] == b[2] for a, b in zip(now, _bn_state(m)))
    # momentum=None is the cumulative average, track_running_stats=False has nothing to move
    m.bn1.momentum = None
    with torch.no_grad():
        m.stem_from_image(x.detach(), batch_stats=True)
    assert int(m.bn1.num_batches_tracked) == 2
    stats = maps["stats"]
    want = now[0][0] * 0.5 + stats[0] * 0.5
    assert torch.allclose(m.bn1.running_mean, want, rtol=1e-6, atol=1e-7)


def test_detector_in_training_mode(gpu):
    m = _fresh(gpu, 6)
    before = _bn_state(m)
    assert len(before) == 20 and len(list(m.parameters())) == 126
    x = torch.randn((2, 3, 32, 64), generator=torch.Generator().manual_seed(3)).to(gpu).requires_grad_()
    out = m.detect_from_image(x, batch_stats=True)
    sum((v * v).sum() + v.sum() for v in out.values()).backward()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    for (rm, rv, nbt), (rm2, rv2, nbt2) in zip(before, _bn_state(m)):
        assert nbt2 == nbt + 1 and not _bits(rm, rm2) and not _bits(rv, rv2)
    # backbone_trainable(batch_stats=True): forward is that call bit for bit with grad on
    m2 = _fresh(gpu, 6)
    m2.backbone_trainable(batch_stats=True)
    out2 = m2(x.detach())
    assert all(v.grad_fn is not None and _bits(v.detach(), out[k].detach()) for k, v in out2.items())
    assert all(a[2] == 1 for a in _bn_state(m2))
    # ... and under no_grad today's fused forward, which moves nothing
    m3 = _fresh(gpu, 6)
    with torch.no_grad():
        plain = m3(x.detach())
        m3.backbone_trainable(batch_stats=True)
        fused = m3(x.detach())
    assert all(_bits(plain[k], fused[k]) for k in plain) and all(a[2] == 0 for a in _bn_state(m3))
    # switched off again, forward with grad on is the fused forward too
    m3.backbone_trainable(False)
    assert all(_bits(plain[k], v) and v.grad_fn is None for k, v in m3(x.detach()).items())
    # one optimiser step, the engine's repack and a second forward (the hand-off to the live handle)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    with torch.no_grad():
        first = m(x.detach())
    opt.step()
    with torch.no_grad():
        second = m(x.detach())
    assert all(torch.isfinite(v).all() for v in second.values())
    assert any(not _bits(first[k], second[k]) for k in first)
    out3 = m.detect_from_image(x.detach(), batch_stats=True)
    assert all(torch.isfinite(v).all() for v in out3.values())


def test_defaults_are_todays_path(gpu, model):
    x = torch.randn((1, 3, 32, 32), generator=torch.Generator().manual_seed(1)).to(gpu)
    saved = _bn_state(model)
    for fn in ("stem_from_image", "detect_from_image"):
        outs = []
        for kw in ({}, dict(batch_stats=False), dict(batch_stats=False, update_running=True)):
            xr = x.clone().requires_grad_()
            for p in model.parameters():
                p.grad = None
            y = getattr(model, fn)(xr, **kw)
            ys = list(y.values()) if isinstance(y, dict) else [y]
            sum(v.square().sum() for v in ys).backward()
            outs.append([v.detach() for v in ys] + [xr.grad] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
        for other in outs[1:]:
            assert len(other) == len(outs[0]) and all(_bits(a, b) for a, b in zip(outs[0], other))
    assert all(_bits(a[0], b[0]) and _bits(a[1], b[1]) and a[2] == b[2] for a, b in zip(saved, _bn_state(model)))


def test_plain_resnet_keeps_refusing(gpu):
    from sfa_hip import dropin  # noqa: F401
    from models.resnet import get_pose_net as plain_net
    m = plain_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False).to(gpu)
    x = torch.zeros((1, 3, 32, 32), device=gpu)
    with pytest.raises(AttributeError):
        m.stem_from_image(x, batch_stats=True)
    with pytest.raises(AttributeError):
        m.backbone_trainable(batch_stats=True)
