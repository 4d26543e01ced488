"""PoseResNet.block_from_input / layers_from_pooled with ``batch_stats=True`` on the GPU: .grad lands on x and on all
6 or 9 parameters and equals the C entries bit for bit, the engine is not called, the running buffers move exactly as
nn.BatchNorm2d moves them in train() (and stay with ``update_running=False``), ``batch_stats=False`` is bit-equal to
the call without the keyword, and the eight chained blocks at the composed, CPU-measured gate of a float64 torch chain."""
import numpy as np
import pytest
import torch

import block_train_restatement as tr
from sfa_hip import runtime

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def model(gpu):
    from models.fpn_resnet import get_pose_net
    import block_restatement as br
    torch.manual_seed(5)
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False).to(gpu)
    own = dict(m.named_parameters())
    own.update(dict(m.named_buffers()))
    for L in (1, 2, 3, 4):
        for b in (0, 1):
            for k, v in br.state_entries(L, b, tr.draw_params(L, b, 700 + 10 * L + b)).items():
                own[k].data.copy_(torch.from_numpy(v))
    return m


def _buffers(mods):
    return [(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)) for _, bn in mods]


def _restore(mods, saved):
    with torch.no_grad():
        for (_, bn), (rm, rv, nbt) in zip(mods, saved):
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
            bn.num_batches_tracked.fill_(nbt)


@pytest.mark.parametrize("layer,block,shape", [(1, 0, (2, 3, 5)), (2, 0, (2, 5, 7)), (4, 1, (1, 2, 3))])
def test_batch_stats_is_the_entries_and_moves_the_running_buffers(gpu, model, layer, block, shape, monkeypatch):
    cin, cout, s, ds = tr.block_shape(layer, block)
    mods = model._block_mods(layer, block)
    assert len(mods) == (3 if ds else 2)
    saved = _buffers(mods)
    for p in model.parameters():
        p.grad = None
    # the training path must not reach the engine (no host repack)
    monkeypatch.setattr(type(model), "_engine", lambda self, device: pytest.fail("batch_stats=True called the engine"))
    gen = torch.Generator().manual_seed(layer * 10 + block)
    B, h, w = shape
    x = torch.randn((B, cin, h, w), generator=gen).to(gpu).requires_grad_()
    try:
        y = model.block_from_input(layer, block, x * 2, batch_stats=True)
        assert tuple(y.shape) == (B, cout, -(-h // s), -(-w // s)) and y.grad_fn is not None
        g = torch.randn(y.shape, generator=gen).to(gpu)
        (y * g).sum().backward()
        torch.cuda.synchronize()
        params = [p for conv, bn in mods for p in (conv.weight, bn.weight, bn.bias)]
        assert len(params) == (9 if ds else 6)
        xn = (x.detach() * 2).permute(0, 2, 3, 1).contiguous()
        m = runtime.block_train_forward(layer, block, xn, [p.detach() for p in params], mods[0][1].eps)
        assert _bits(y.detach().permute(0, 2, 3, 1), m["y"])
        dx, dp = runtime.block_train_grad(layer, block, xn, m, g.permute(0, 2, 3, 1).contiguous(), [p.detach() for p in params],
                                          mods[0][1].eps)
        assert x.grad is not None and _bits(x.grad, dx.permute(0, 3, 1, 2) * 2)
        for p, d in zip(params, dp):
            assert p.grad is not None and p.grad.shape == p.shape and _bits(p.grad, d)
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
        # the running buffers: nn.BatchNorm2d in train() on the device's own z maps
        n = B * m["y"].shape[1] * m["y"].shape[2]
        for i, ((_, bn), (rm, rv, nbt), zk) in enumerate(zip(mods, saved, ("z1", "z2", "zd"))):
            ref = torch.nn.BatchNorm2d(cout, eps=bn.eps, momentum=bn.momentum).double().train()
            ref.running_mean.copy_(rm.double().cpu())
            ref.running_var.copy_(rv.double().cpu())
            ref(m[zk].permute(0, 3, 1, 2).double().cpu())
            assert int(bn.num_batches_tracked) == nbt + 1
            # float32 statistics (u relative, stats_stage's bound) through a float32 update of three roundings
            st = m["stats"].cpu().numpy().astype(np.float64)
            (mean, var), (Em, Ev) = tr.stats_stage(m[zk].cpu().numpy())
            for which, (buf, rbuf, before, E) in enumerate(((bn.running_mean, ref.running_mean, rm, Em),
                                                            (bn.running_var, ref.running_var, rv, Ev))):
                bound = tr.running_bound(before.cpu().numpy(), st[i, which], E, n, which)
                assert tr.ratio(buf.cpu().numpy(), rbuf.numpy(), bound) <= 1.0, (i, which)
                assert not _bits(buf, before), "a running buffer did not move"
        # update_running=False leaves them alone
        now = _buffers(mods)
        with torch.no_grad():
            y2 = model.block_from_input(layer, block, x.detach() * 2, batch_stats=True, update_running=False)
        assert _bits(y2, y.detach())
        for (rm, rv, nbt), (_, bn) in zip(now, mods):
            assert _bits(rm, bn.running_mean) and _bits(rv, bn.running_var) and int(bn.num_batches_tracked) == nbt
    finally:
        _restore(mods, saved)


def test_batch_stats_false_is_todays_path(gpu, model):
    x = torch.randn((2, 64, 4, 6), generator=torch.Generator().manual_seed(1)).to(gpu)
    mods = model._block_mods(2, 0)
    saved = _buffers(mods)
    outs = []
    for kw in ({}, dict(batch_stats=False), dict(batch_stats=False, update_running=True)):
        xr = x.clone().requires_grad_()
        for p in model.parameters():
            p.grad = None
        y = model.block_from_input(2, 0, xr, **kw)
        y.square().sum().backward()
        outs.append([y.detach(), xr.grad] + [p.grad.clone() for conv, bn in mods for p in (conv.weight, bn.weight, bn.bias)])
    for other in outs[1:]:
        assert all(_bits(a, b) for a, b in zip(outs[0], other))
    for (rm, rv, nbt), (_, bn) in zip(saved, mods):
        assert _bits(rm, bn.running_mean) and _bits(rv, bn.running_var) and int(bn.num_batches_tracked) == nbt
    with torch.no_grad():
        a = model.layers_from_pooled(torch.randn((1, 64, 8, 8), generator=torch.Generator().manual_seed(2)).to(gpu))
        b = model.layers_from_pooled(torch.randn((1, 64, 8, 8), generator=torch.Generator().manual_seed(2)).to(gpu),
                                     batch_stats=False)
    assert all(_bits(u, v) for u, v in zip(a, b))


def test_layers_from_pooled_at_the_composed_gate(gpu):
    """layers_from_pooled(x, batch_stats=True) at (2, 64, 16, 24) through L = sum <g_L, out_layer_L> and backward():
    out_layer1..4, the gradients at x and all 57 block parameters and the 38 running buffers after the step, each at
    gate(t) = 4 (noise32(t) + perturb(t)) of the float64 torch chain with F.batch_norm(training=True)
    (tests/block_train_chain.py), both forms of the metric.  The gate was measured on the CPU
    (tests/golden/gen_block_train_chain_golden.py) and is at most 4.4e-3; tests/test_block_train_chain_host.py shows
    that running statistics miss it by 3.9e6x, a dropped skip gradient by 3.3e3x and a BatchNorm backward without its
    sum dY x^ term by 2.0e3x."""
    import block_train_chain as bc
    from models.fpn_resnet import get_pose_net
    from test_block_train_chain_host import reference
    g, sd, ref, gate, _ = reference()
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False).to(gpu)
    own = dict(m.named_parameters())
    own.update(dict(m.named_buffers()))
    for k, v in sd.items():
        own[k].data.copy_(torch.from_numpy(v))
    x = torch.from_numpy(g["x"]).to(gpu).requires_grad_()
    outs = m.layers_from_pooled(x, batch_stats=True)
    assert [tuple(o.shape) for o in outs] == [(2, 64, 16, 24), (2, 128, 8, 12), (2, 256, 4, 6), (2, 512, 2, 3)]
    sum((o * torch.from_numpy(c).to(gpu)).sum() for o, c in zip(outs, bc.cotangents())).backward()
    torch.cuda.synchronize()
    got = {n: o.detach().cpu().numpy() for n, o in zip(bc.LAYERS, outs)}
    got["grad/x"] = x.grad.cpu().numpy()
    names = bc.parameter_names(sd)
    assert len(names) == 57 and {id(own[k]) for k in names} == {id(p) for p in m.block_parameters()}
    for k in names:
        assert own[k].grad is not None, k
        got["grad/" + k] = own[k].grad.cpu().numpy()
    for k in sd:
        if k.endswith(("running_mean", "running_var")):
            got[k] = own[k].cpu().numpy()
            assert int(own[k.rsplit(".", 1)[0] + ".num_batches_tracked"]) == 1
    q, k, each = bc.worst(got, ref, gate)
    groups = {"out": [v for n, v in each.items() if n.startswith("out_")], "grad x": [each["grad/x"]],
              "grad parameters": [v for n, v in each.items() if n.startswith("grad/l")],
              "running": [v for n, v in each.items() if "running" in n]}
    print("layers_from_pooled(batch_stats=True): worst m / gate " + "  ".join(f"{n} {max(v):.3f}" for n, v in groups.items()) +
          f"  (worst at {k})")
    assert q <= 1.0, (q, k)
