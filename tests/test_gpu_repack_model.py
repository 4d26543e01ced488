"""The model keeps its engine across weight updates (PoseResNet._engine -> KfpnEngine.repack): the same handle and
the bits of the host route after in-place updates, three Adam steps, a captured forward graph and a twin replayed
after a repack, the refusal of a stale backward, and the cases that still take the host route.  Every comparison
is equality against the host pack route (fpn_resnet._DEVICE_REPACK off).  Batch 2 at 64 x 64 and 96 x 96."""
import contextlib

import numpy as np
import pytest
import torch

from sfa_hip import _lib, runtime, synthetic

pytestmark = pytest.mark.gpu

B = 2
# one parameter of every unit kind (stem, body conv, downsample segment, a BatchNorm, FPN conv, head 3x3 / 1x1 / bias)
# and one running buffer
TOUCHED = ("conv1.weight", "layer1.0.conv1.weight", "layer2.0.downsample.0.weight", "layer2.0.bn2.weight",
           "conv_up_level1.weight", "fpn0_hm_cen.0.weight", "fpn1_dim.2.weight", "fpn2_z_coor.2.bias",
           "layer3.1.bn1.running_mean")


@pytest.fixture(autouse=True)
def _grad_mode():
    with torch.enable_grad():
        yield


@contextlib.contextmanager
def host_route():
    from models import fpn_resnet
    old = fpn_resnet._DEVICE_REPACK[0]
    fpn_resnet._DEVICE_REPACK[0] = False
    try:
        yield
    finally:
        fpn_resnet._DEVICE_REPACK[0] = old


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _make(gpu, state=None, seed=4):
    from models.fpn_resnet import get_pose_net
    model = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False)
    if state is None:
        sd = synthetic.synthetic_state_dict(_lib.state_layout(model._arch), seed)
        state = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    model.load_state_dict(state, strict=False)
    return model.to(gpu).eval()


def _input(gpu, size, seed=3):
    return torch.from_numpy(synthetic.synthetic_bev(B, size, size, seed=seed)).to(gpu)


def _touch(model, names=TOUCHED, step=0.01):
    sd = model.state_dict(keep_vars=True)
    with torch.no_grad():
        for n in names:
            sd[n].add_(step)


def _configure(model, gpu, config):
    if config == "fp16":
        model.set_math("fp16")
    eng = model._engine(gpu)
    if config == "images_off":
        eng.set_option(_lib.OPT_W_IMAGES, 0)
    return eng


def _host_reference(model, gpu, x, config):
    """The maps of a fresh model loaded from model's state_dict, its engine packed on the host."""
    with host_route(), torch.no_grad():
        fresh = _make(gpu, {k: v.detach().cpu() for k, v in model.state_dict().items()})
        _configure(fresh, gpu, config)
        want = {k: v.clone() for k, v in fresh(x).items()}
    return want


@pytest.mark.parametrize("size", [64, 96])
@pytest.mark.parametrize("config", ["default", "images_off", "fp16"])
def test_kept_handle_same_numbers(gpu, size, config):
    model = _make(gpu)
    x = _input(gpu, size)
    eng = _configure(model, gpu, config)
    with torch.no_grad():
        before = {k: v.clone() for k, v in model(x).items()}
    _touch(model)
    assert model._engine(gpu) is eng
    with torch.no_grad():
        got = {k: v.clone() for k, v in model(x).items()}
    assert model._engine(gpu) is eng
    want = _host_reference(model, gpu, x, config)
    torch.cuda.synchronize()
    assert list(got) == list(want) and all(_bits(got[k], want[k]) for k in want)
    assert not all(_bits(got[k], before[k]) for k in want)


def _adam_loop(gpu, size, steps=3):
    from losses.losses import Compute_Loss
    model = _make(gpu).backbone_trainable()
    x = _input(gpu, size)
    tb = runtime.TargetBuilder(gpu, hm_size=(size // 4, size // 4))
    tg = tb(*synthetic.synthetic_labels(B, seed=2))
    crit = Compute_Loss(gpu, differentiable=True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0)
    losses, engines = [], []
    for _ in range(steps):
        opt.zero_grad()
        total, _ = crit(dict(model(x)), tg)
        engines.append(model._engine(gpu))
        losses.append(total.detach().clone())
        total.backward()
        opt.step()
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in model.parameters()], engines


def test_three_adam_steps_equal_the_host_route(gpu):
    losses, params, engines = _adam_loop(gpu, 64)
    assert all(e is engines[0] for e in engines)
    with host_route():
        want_losses, want_params, want_engines = _adam_loop(gpu, 64)
    assert len({id(e) for e in want_engines}) == len(want_engines)  # the host route builds a new engine per step
    assert all(_bits(a, b) for a, b in zip(losses, want_losses))
    assert len(params) == 126 and all(_bits(a, b) for a, b in zip(params, want_params))
    assert not _bits(losses[0], losses[-1])


def _capture(eng, x, outs, ws):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.forward_into(x, outs, _lib.IN_NCHW3, ws, _lib.stream_ptr(x.device))
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.forward_into(x, outs, _lib.IN_NCHW3, ws, _lib.stream_ptr(x.device))
    return g


def test_captured_graphs_survive_a_repack(gpu):
    size = 96
    model = _make(gpu)
    x = _input(gpu, size)
    with torch.cuda.device(gpu), torch.no_grad():
        eng = model._engine(gpu)
        twin = eng.twin()
        runs = []
        for e in (eng, twin):
            outs = e.alloc_outputs(B, size, size)
            ws = torch.empty(e.workspace_bytes(B, size, size), dtype=torch.uint8, device=gpu)
            runs.append((_capture(e, x, outs, ws), outs, ws))
        _touch(model)
        assert model._engine(gpu) is eng  # repacks on the current stream
        got = []
        for g, outs, _ in runs:
            for t in outs.values():
                t.zero_()
            g.replay()
            torch.cuda.synchronize()
            got.append({k: v.clone() for k, v in outs.items()})
    want = _host_reference(model, gpu, x, "default")
    for maps in got:
        assert all(_bits(maps[k], want[k]) for k in want)


def test_stale_backward_is_refused(gpu):
    model = _make(gpu).backbone_trainable()
    x = _input(gpu, 64)
    first = sum((t * t).mean() for t in model(x).values())
    with torch.no_grad():
        model.fpn1_dim[0].weight.add_(0.01)
    model(x)
    with pytest.raises(RuntimeError):
        first.backward()


def test_stale_backward_is_refused_for_a_neck_weight_alone(gpu):
    """neck_trainable(): sfa_model_neck_grad's data gradients read conv_up_level2 / 3's packed weights, which the
    repack rewrites in place; a change of that weight alone refuses the pending backward."""
    for name in ("conv_up_level2", "conv_up_level3"):
        model = _make(gpu).neck_trainable()
        x = _input(gpu, 64)
        first = sum((t * t).mean() for t in model(x).values())
        assert first.grad_fn is not None
        with torch.no_grad():
            getattr(model, name).weight.add_(0.01)
        model(x)
        with pytest.raises(RuntimeError):
            first.backward()
    model = _make(gpu).neck_trainable()  # the same sequence with a block's running buffer: no weight of its calls moved
    first = sum((t * t).mean() for t in model(x).values())
    with torch.no_grad():
        model.layer2[0].bn1.running_mean.add_(0.01)
    model(x)
    first.backward()
    torch.cuda.synchronize()
    assert model.conv_up_level2.weight.grad is not None


def test_a_moved_running_buffer_does_not_stale_the_stem_or_the_neck(gpu):
    model = _make(gpu)
    x = _input(gpu, 64)
    pooled = model.stem_from_image(x)
    maps = model.detect_from_layers(*[t.detach() for t in model.layers_from_pooled(pooled.detach())])
    eng = model._engine(gpu)
    with torch.no_grad():
        model.layer2[0].bn1.running_mean.add_(0.01)
        model(x)  # the second forward: it repacks the engine in place
    assert model._engine(gpu) is eng
    (pooled * pooled).mean().backward()
    sum((t * t).mean() for t in maps.values()).backward()
    torch.cuda.synchronize()
    assert model.conv1.weight.grad is not None and model.conv_up_level1.weight.grad is not None


def test_batch_stats_forward_keeps_one_engine(gpu):
    def run(update_running):
        model = _make(gpu)
        x = torch.from_numpy(synthetic.synthetic_bev(B, 64, 64, seed=5)).to(gpu)
        pooled = model.stem_from_image(x)
        eng = model._engine(gpu)
        outs = model.detect_from_pooled(pooled, batch_stats=True, update_running=update_running)
        assert model._engine(gpu) is eng
        sum((t * t).mean() for t in outs.values()).backward()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in model.parameters()]

    moved, still = run(True), run(False)
    assert len(moved) == 126 and all(_bits(a, b) for a, b in zip(moved, still))


def test_fallbacks(gpu):
    x = _input(gpu, 64)
    # load_state_dict copies in place (the same pointers, new versions): a repack
    model = _make(gpu)
    eng = model._engine(gpu)
    other = synthetic.synthetic_state_dict(_lib.state_layout(model._arch), 9)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in other.items()}, strict=False)
    assert model._engine(gpu) is eng
    with torch.no_grad():
        got = model(x)
    want = _host_reference(model, gpu, x, "default")
    assert all(_bits(got[k], want[k]) for k in want)
    # .to(gpu) after an engine over CPU-resident weights: moved tensors, the host route's new engine
    from models.fpn_resnet import get_pose_net
    cpu = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, imagenet_pretrained=False).eval()
    cpu.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in other.items()}, strict=False)
    with torch.no_grad():
        on_host = cpu(x)
        e0 = cpu._engine(gpu)
        cpu.to(gpu)
        moved = cpu(x)
    assert cpu._engine(gpu) is not e0
    assert all(_bits(on_host[k], want[k]) and _bits(moved[k], want[k]) for k in want)
    # a float64 parameter: the host route on every change
    model.conv1.weight.data = model.conv1.weight.data.double()
    with torch.no_grad():
        e1 = model._engine(gpu)
        model.conv1.weight.add_(0.0)
        wide = model(x)
    assert model._engine(gpu) is not e1 and e1 is not eng
    assert all(_bits(wide[k], want[k]) for k in want)


RESNET_TOUCHED = ("conv1.weight", "layer4.0.downsample.1.bias", "deconv_layers.0.weight", "deconv_layers.3.weight",
                  "deconv_layers.1.weight", "deconv_layers.7.running_var", "hm_cen.0.weight", "dim.2.weight", "z_coor.2.bias")


def test_resnet_18_keeps_its_handle(gpu):
    import headset_cases as hc
    heads = dict(runtime.DEFAULT_HEADS)
    model, _ = hc.make_model("resnet_18", heads, gpu)
    x = _input(gpu, 96)
    eng = model._engine(gpu)
    with torch.no_grad():
        before = {k: v.clone() for k, v in model(x).items()}
    _touch(model, RESNET_TOUCHED)
    with torch.no_grad():
        got = {k: v.clone() for k, v in model(x).items()}
    assert model._engine(gpu) is eng
    with host_route(), torch.no_grad():
        fresh, _ = hc.make_model("resnet_18", heads, gpu)
        fresh.load_state_dict(model.state_dict())
        want = {k: v.clone() for k, v in fresh(x).items()}
    torch.cuda.synchronize()
    assert list(got) == list(want) and all(_bits(got[k], want[k]) for k in want)
    assert not all(_bits(got[k], before[k]) for k in want)


def test_an_unindexed_device_takes_the_device_route(gpu):
    model = _make(gpu)
    tensors = list(model.state_dict(keep_vars=True).values())
    with torch.cuda.device(gpu):
        assert runtime.device_packable(tensors, "cuda") and runtime.device_packable(tensors, torch.device("cuda"))
    assert runtime.device_packable(tensors, gpu) and not runtime.device_packable(tensors, "cpu")


def test_a_failed_repack_leaves_no_stale_engine(gpu, monkeypatch):
    model = _make(gpu)
    x = _input(gpu, 64)
    eng = model._engine(gpu)
    _touch(model)

    def fail(self, tensors, stream=None):
        raise ValueError("repack failed")

    monkeypatch.setattr(runtime.KfpnEngine, "repack", fail)
    with pytest.raises(ValueError):
        model._engine(gpu)
    monkeypatch.undo()
    with torch.no_grad():
        got = model(x)
    assert model._engine(gpu) is not eng  # the engine whose repack failed is gone
    want = _host_reference(model, gpu, x, "default")
    assert all(_bits(got[k], want[k]) for k in want)
