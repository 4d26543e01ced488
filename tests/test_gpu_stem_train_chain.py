"""stem_from_image + layers_from_pooled with ``batch_stats=True`` at (2, 3, 64, 96) through
L = sum <g_L, out_layer_L> and backward(): out_layer1..4, the gradients at x and all 60 stem and block parameters and
the 40 running buffers after the step, each at gate(t) = 4 (noise32(t) + perturb(t)) of the float64 torch chain
(tests/stem_train_chain.py), both forms of the metric.  The gate was measured on the CPU
(tests/golden/gen_stem_train_chain_golden.py); tests/test_stem_train_chain_host.py shows what misses it."""
import pytest
import torch

import stem_train_chain as sc
from sfa_hip import runtime

pytestmark = pytest.mark.gpu


def test_chain_from_the_image_at_the_composed_gate(gpu):
    from models.fpn_resnet import get_pose_net
    from test_stem_train_chain_host import reference
    g, sd, ref, gate, _ = reference()
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False).to(gpu)
    own = dict(m.named_parameters())
    own.update(dict(m.named_buffers()))
    for k, v in sd.items():
        own[k].data.copy_(torch.from_numpy(v))
    with torch.enable_grad():
        x = torch.from_numpy(g["x"]).to(gpu).requires_grad_()
        outs = m.layers_from_pooled(m.stem_from_image(x, batch_stats=True), batch_stats=True)
        assert [tuple(o.shape) for o in outs] == [(2, 64, 16, 24), (2, 128, 8, 12), (2, 256, 4, 6), (2, 512, 2, 3)]
        sum((o * torch.from_numpy(c).to(gpu)).sum() for o, c in zip(outs, sc.cotangents())).backward()
    torch.cuda.synchronize()
    got = {n: o.detach().cpu().numpy() for n, o in zip(sc.LAYERS, outs)}
    got["grad/x"] = x.grad.cpu().numpy()
    names = sc.parameter_names(sd)
    assert len(names) == 60 and {id(own[k]) for k in names} == {id(p) for p in m.stem_parameters() + m.block_parameters()}
    for k in names:
        assert own[k].grad is not None, k
        got["grad/" + k] = own[k].grad.cpu().numpy()
    for k in sd:
        if k.endswith(("running_mean", "running_var")):
            got[k] = own[k].cpu().numpy()
            assert int(own[k.rsplit(".", 1)[0] + ".num_batches_tracked"]) == 1
    q, k, each = sc.worst(got, ref, gate)
    groups = {"out": [v for n, v in each.items() if n.startswith("out_")], "grad x": [each["grad/x"]],
              "grad stem": [v for n, v in each.items() if n.startswith(("grad/conv1", "grad/bn1"))],
              "grad blocks": [v for n, v in each.items() if n.startswith("grad/l")],
              "running": [v for n, v in each.items() if "running" in n]}
    print("chain from the image (batch_stats=True): worst m / gate " + "  ".join(f"{n} {max(v):.3f}" for n, v in groups.items()) +
          f"  (worst at {k})")
    assert q <= 1.0, (q, k)
