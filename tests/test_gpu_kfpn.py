"""sfa_kfpn_combine / sfa_kfpn_combine_grad on the GPU: against the reference fixture (tests/golden/gen_kfpn_golden.py),
the float64 restatement (tests/kfpn_restatement.py) and the model's own fused combine; the autograd Function behind
PoseResNet.apply_kfpn and runtime.kfpn_heads; the chain into the differentiable Compute_Loss.

Bounds.  Forward: the project's per-kernel gate, <= 1e-5 max(1, |ref|), against the reference; bit-identity with the
model's head maps and between the vector and scalar kernels.  Gradient: kfpn_restatement's derived bound
(GRAD_REL |r| + GRAD_ABS sum_children |g| (1 + max|v|) + GRAD_FLOOR) against the restatement, that plus the
fixture's d_ref against the reference's float32 autograd; exact zeros where a weight is exactly 0."""
import numpy as np
import pytest
import torch

import golden_cases as gc
import golden_io
import kfpn_restatement as kr
from conftest import GOLDEN
from sfa_hip import runtime
from test_kfpn_host import CASES, case_inputs, zero_weight_masks

pytestmark = pytest.mark.gpu


class Cfg(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def g():
    return golden_io.load(GOLDEN, "kfpn_golden")


def _offset_view(t):
    """The same values at an address that is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    buf.copy_(t)
    assert buf.data_ptr() % 16 == 4 and buf.is_contiguous()
    return buf


def _dev(levels, gpu, shifted=False):
    put = (lambda v: _offset_view(torch.from_numpy(np.ascontiguousarray(v)).to(gpu))) if shifted else (
        lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(gpu))
    return {h: [put(v) for v in lv] if isinstance(lv, (list, tuple)) else put(lv) for h, lv in levels.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _random_levels(heads, B, h, w, half, seed):
    rng = np.random.default_rng(seed)
    lv = {n: [(rng.standard_normal((B, c, h // 2, w // 2) if half else (B, c, h, w)) * 2).astype(np.float32),
              (rng.standard_normal((B, c, h, w)) * 2).astype(np.float32),
              (rng.standard_normal((B, c, h, w)) * 2).astype(np.float32)] for n, c in heads.items()}
    up = {n: rng.standard_normal((B, c, h, w)).astype(np.float32) for n, c in heads.items()}
    return lv, up


def _check_forward(tag, got_out, got_w, ref_out, ref_w):
    for what, got, ref in (("out", got_out, ref_out), ("weights", got_w, ref_w)):
        got = got.cpu().numpy()
        assert got.shape == ref.shape
        err = np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
        print(f"kfpn[{tag}] {what}: max gated error {err.max():.3e}")
        assert err.max() <= kr.GATE, (tag, what, err.max())


def _check_grad(tag, got, levels, up, half, ref=None, d_ref=None):
    """got: three GPU tensors of one head.  Returns the largest error / bound against the restatement."""
    mine, absolute = kr.grad(levels, up, half), kr.grad_bound(levels, up, half)
    worst = 0.0
    for l in range(3):
        x = got[l].cpu().numpy()
        assert x.shape == mine[l].shape and not np.isnan(x).any()
        ok, ratio = kr.within(x, mine[l], absolute[l])
        worst = max(worst, ratio)
        print(f"kfpn_grad[{tag}] level {l}: max |gpu - restatement| {np.abs(x - mine[l]).max():.3e}, "
              f"max error / bound {ratio:.3e}")
        assert ok, (tag, l, ratio)
        if ref is not None:
            err = np.abs(x.astype(np.float64) - ref[l])
            print(f"kfpn_grad[{tag}] level {l}: max |gpu - reference| {err.max():.3e}, d_ref {d_ref[l]:.3e}")
            assert np.all(err <= kr.GRAD_REL * np.abs(mine[l]) + absolute[l] + d_ref[l]), (tag, l)
    return worst


@pytest.mark.parametrize("name", CASES)
def test_forward_matches_the_reference_and_the_two_forms_agree(g, gpu, name):
    heads, half, lv, _ = case_inputs(g, name)
    out, wts = runtime.kfpn_combine(_dev(lv, gpu), half, return_weights=True)
    for h in heads:
        _check_forward(f"{name}/{h}", out[h], wts[h], g[f"{name}/out/{h}"], g[f"{name}/weights/{h}"])
    # every base one float past a 16-byte boundary: the scalar kernel, the same bits; and without the weights
    sh_out = {h: _offset_view(torch.empty_like(out[h])) for h in heads}
    sh_w = {h: _offset_view(torch.empty_like(wts[h])) for h in heads}
    runtime.kfpn_combine(_dev(lv, gpu, shifted=True), half, out=sh_out, weights=sh_w)
    alone = runtime.kfpn_combine(_dev(lv, gpu), half)
    for h in heads:
        assert _same_bits(out[h], sh_out[h]) and _same_bits(wts[h], sh_w[h]) and _same_bits(out[h], alone[h]), h


def test_forward_is_bit_identical_to_the_models_fused_combine(golden, gpu):
    from models.model_utils import create_model
    model = create_model(Cfg(arch="fpn_resnet_18", heads=dict(gc.HEADS), head_conv=64, imagenet_pretrained=False))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in gc.state_dict_np(golden.model).items()})
    model = model.to(gpu).eval()
    model.capture_visualization = True
    with torch.no_grad():
        outs = model(torch.from_numpy(gc.model_input("b2_96")).to(gpu))
    levels = {}
    for h, lv in model.get_visualization_data()["fpn_outputs"].items():
        # the capture repeats level 0 up to H/4 x W/4: back to the half resolution the heads produce
        levels[h] = [lv[0][:, :, ::2, ::2].contiguous(), lv[1].contiguous(), lv[2].contiguous()]
    assert list(levels) == list(gc.HEADS) and levels["hm_cen"][0].shape == (2, 3, 12, 12)
    got = runtime.kfpn_heads(levels, level0_half=True)
    for h in gc.HEADS:
        assert got[h].shape == outs[h].shape and _same_bits(got[h], outs[h]), h
        assert bool((outs[h] != 0).any())


@pytest.mark.parametrize("name", CASES)
def test_gradient_matches_the_restatement_and_the_reference(g, gpu, name):
    heads, half, lv, up = case_inputs(g, name)
    got = runtime.kfpn_combine_grad(_dev(lv, gpu), _dev(up, gpu), half)
    shifted = runtime.kfpn_combine_grad(_dev(lv, gpu, shifted=True), _dev(up, gpu, shifted=True), half)
    for h in heads:
        ref = [g[f"{name}/grad/{h}/{l}"] for l in range(3)]
        _check_grad(f"{name}/{h}", got[h], lv[h], up[h], half, ref, g[f"{name}/d_ref"])
        masks = zero_weight_masks(g, name, h, half)
        for l in range(3):
            x = got[h][l].cpu().numpy()
            assert np.all(x[masks[l]] == 0), (name, h, l)  # exactly 0 where the weight is exactly 0
            assert _same_bits(got[h][l], shifted[h][l]), (name, h, l)  # vector and scalar kernels
        if name == "saturated":
            assert all(m.any() for m in masks)


@pytest.mark.parametrize("half", [True, False])
def test_three_frames_eleven_channels(gpu, half):
    """B 3, 11 channels in two heads at 10 x 12 (level 0 at 5 x 6): more than one frame and head, rows of 3 pairs."""
    lv, up = _random_levels({"a": 5, "b": 6}, 3, 10, 12, half, 11)
    out, wts = runtime.kfpn_combine(_dev(lv, gpu), half, return_weights=True)
    got = runtime.kfpn_combine_grad(_dev(lv, gpu), _dev(up, gpu), half)
    for h in lv:
        _check_forward(f"3x11/{h}", out[h], wts[h], *kr.forward(lv[h], half))
        _check_grad(f"3x11/{h}", got[h], lv[h], up[h], half)


def test_152_the_workloads_head_map(gpu):
    """152 x 152, B 2, the five heads, level 0 at 76 x 76: 23 blocks per (frame, channel) in the forward."""
    lv, up = _random_levels(gc.HEADS, 2, 152, 152, True, 12)
    out, wts = runtime.kfpn_combine(_dev(lv, gpu), True, return_weights=True)
    got = runtime.kfpn_combine_grad(_dev(lv, gpu), _dev(up, gpu), True)
    for h in lv:
        _check_forward(f"152/{h}", out[h], wts[h], *kr.forward(lv[h], True))
        _check_grad(f"152/{h}", got[h], lv[h], up[h], True)


def test_runs_are_bit_identical_and_every_byte_is_written(gpu):
    lv, up = _random_levels({"a": 3, "b": 2, "c": 1}, 2, 24, 40, True, 13)
    dl, du = _dev(lv, gpu), _dev(up, gpu)
    a = runtime.kfpn_combine_grad(dl, du, True)
    b = runtime.kfpn_combine_grad(dl, du, True)
    out = {h: [torch.empty_like(t) for t in v] for h, v in dl.items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        runtime.kfpn_combine_grad(dl, du, True, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        runtime.kfpn_combine_grad(dl, du, True, out=out)
    for v in out.values():
        for t in v:
            t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for h in dl:
        for l in range(3):
            assert not torch.isnan(out[h][l]).any(), (h, l)  # every byte is written by the kernel
            assert _same_bits(a[h][l], b[h][l]) and _same_bits(a[h][l], out[h][l]), (h, l)
            assert bool((a[h][l] != 0).any())


def test_apply_kfpn_autograd(gpu):
    from models import fpn_resnet
    model = fpn_resnet.get_pose_net(18, dict(gc.HEADS), 64, False)
    lv, _ = _random_levels({"head": 3}, 2, 6, 8, False, 14)
    ones = {"head": torch.ones(2, 3, 6, 8, device=gpu)}
    want = runtime.kfpn_combine_grad(_dev(lv, gpu), ones)["head"]
    plain, plain_w = runtime.kfpn_combine(_dev(lv, gpu), return_weights=True)
    for factor in (1.0, 0.5):
        a, b, c = (t.requires_grad_(True) for t in _dev(lv, gpu)["head"])
        out, weights = model.apply_kfpn([a, b, c])
        assert out.requires_grad and not weights.requires_grad and weights.shape == (2, 3, 6, 8, 3)
        assert _same_bits(out.detach(), plain["head"]) and _same_bits(weights, plain_w["head"])
        (out.sum() * factor).backward()
        for leaf, w in zip((a, b, c), want):
            assert _same_bits(leaf.grad, w * factor), factor  # a factor of 0.5 halves it exactly
    # a level that does not require grad gets none; no level requiring grad: no graph
    a, b, c = _dev(lv, gpu)["head"]
    b.requires_grad_(True)
    out, _ = model.apply_kfpn([a, b, c])
    out.sum().backward()
    assert a.grad is None and c.grad is None and _same_bits(b.grad, want[1])
    out, _ = model.apply_kfpn(_dev(lv, gpu)["head"])
    assert not out.requires_grad


def test_chain_into_the_differentiable_loss(gpu):
    """kfpn_heads -> Compute_Loss(differentiable=True) -> backward, at loss_grad_golden's generic shape: the level
    gradients are LossEvaluator.grad followed by kfpn_combine_grad, bit for bit."""
    import loss_restatement as lr
    from losses.losses import Compute_Loss
    lg = golden_io.load(GOLDEN, "loss_grad_golden")
    tg = {k: torch.from_numpy(np.ascontiguousarray(lg[f"generic/t/{k}"])).to(gpu) for k in lr.KEYS}
    B, C, H, W = lg["generic/logits/hm_cen"].shape
    heads = dict(runtime.DEFAULT_HEADS, hm_cen=C)
    lv, _ = _random_levels(heads, B, H, W, True, 15)
    leaves = {h: [t.requires_grad_(True) for t in v] for h, v in _dev(lv, gpu).items()}
    outs = runtime.kfpn_heads(leaves, level0_half=True)
    total, _ = Compute_Loss(gpu, differentiable=True)(dict(outs), tg)
    total.backward()

    maps = runtime.kfpn_combine(_dev(lv, gpu), True)
    at_heads = runtime.LossEvaluator(gpu).grad(maps, tg, apply_sigmoid=True)
    want = runtime.kfpn_combine_grad(_dev(lv, gpu), at_heads, True)
    for h in heads:
        assert _same_bits(outs[h].detach(), maps[h]), h
        for l in range(3):
            assert leaves[h][l].grad.shape == leaves[h][l].shape
            assert _same_bits(leaves[h][l].grad, want[h][l]), (h, l)
    assert any(bool((t.grad != 0).any()) for v in leaves.values() for t in v)
