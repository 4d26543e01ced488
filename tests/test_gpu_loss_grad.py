"""sfa_compute_loss_grad against the float64 closed form (tests/loss_grad_restatement.py) and the reference's
autograd gradients (tests/golden/gen_loss_grad_golden.py); LossEvaluator.grad and the differentiable Compute_Loss.

Bounds, per element.  apply_sigmoid = 0: |gpu - restatement| <= 1e-6 |g| — the same float32 operands, float64 on
both sides, sums of at most M like-sized terms, one rounding to float32 (6e-8); zeros are exact zeros.
apply_sigmoid = 1: that plus the change of the restatement's gradient when s moves by up to 2 float32 ulp, the
accuracy of the device's sigmoid, computed by the restatement.  Against the
reference: that plus d_ref = |reference - restatement| from the fixture (the triangle inequality)."""
import numpy as np
import pytest
import torch

import golden_io
import loss_grad_restatement as gr
import loss_restatement as lr
from conftest import GOLDEN
from sfa_hip import runtime, synthetic
from test_loss_grad_host import CASES, HEADS, SIG, case_inputs, probabilities

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return golden_io.load(GOLDEN, "loss_grad_golden")


def _dev(d, gpu):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in d.items()}


def _host(d):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in d.items()}


def _offset_view(t):
    """The same values at an address that is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    buf.copy_(t)
    assert buf.data_ptr() % 16 == 4 and buf.is_contiguous()
    return buf


def _operands(name, preds, gpu):
    d = _dev(preds, gpu)
    if name == "nonsquare":  # the scalar instantiation: hm_cen and one regression map off the 16-byte grid
        d["hm_cen"], d["dim"] = _offset_view(d["hm_cen"]), _offset_view(d["dim"])
    return d


@pytest.mark.parametrize("name", CASES)
def test_probability_gradients_match_the_restatement(g, gpu, name):
    logits, tg, s, _ = case_inputs(g, name)
    preds = probabilities(logits, s)
    got = _host(runtime.LossEvaluator(gpu).grad(_operands(name, preds, gpu), _dev(tg, gpu)))
    mine = gr.compute_loss_grad(preds, tg)
    for h in HEADS:
        err = np.abs(got[h] - mine[h])
        rel = np.max(err / np.maximum(np.abs(mine[h]), 1e-300))
        print(f"loss_grad[{name}/{h}] apply_sigmoid=0: max rel. error {rel:.3e}")
        assert np.all(err <= 1e-6 * np.abs(mine[h])), (name, h, rel)
        assert np.all(got[h][mine[h] == 0] == 0)


@pytest.mark.parametrize("name", CASES)
def test_logit_gradients_match_the_restatement_and_the_reference(g, gpu, name):
    logits, tg, s, ref = case_inputs(g, name)
    got = _host(runtime.LossEvaluator(gpu).grad(_operands(name, logits, gpu), _dev(tg, gpu), apply_sigmoid=True))
    mine, slack = gr.sigmoid_slack(logits, tg, s)
    for h in HEADS:
        bound = 1e-6 * np.abs(mine[h]) + slack[h]
        err, d_ref = np.abs(got[h] - mine[h]), np.abs(ref[h].astype(np.float64) - mine[h])
        print(f"loss_grad[{name}/{h}] apply_sigmoid=1: max error / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}, "
              f"max |gpu - ref| {np.abs(got[h] - ref[h]).max():.3e}, max d_ref {d_ref.max():.3e}")
        assert np.all(err <= bound), (name, h)
        assert np.all(np.abs(got[h] - ref[h]) <= bound + d_ref), (name, h)
    if name == "saturated":
        for h in SIG:
            out = (s[h] < gr.LO) | (s[h] > gr.HI)
            assert out.any() and np.all(got[h][out] == 0)


def _synthetic_case(B, H, W, C=3, M=50, seed=5):
    labels, offsets = synthetic.synthetic_labels(B, seed=seed)
    tg, _ = lr.build_targets_batch(labels, offsets, [b % 2 == 1 for b in range(B)], hm_size=(H, W), num_classes=C,
                                   max_objects=M)
    logits = {h: synthetic.synthetic_logits((B, c, H, W), seed, 40 + i, 2.0)
              for i, (h, c) in enumerate(zip(HEADS, (C, 2, 2, 1, 3)))}
    return logits, tg


@pytest.fixture(scope="module")
def big():
    return _synthetic_case(2, 152, 152)


def test_152_matches_the_restatement(gpu, big):
    """152 x 152, B = 2, M = 50: 23 blocks per frame (the last one partial) and 34 count partials to fold."""
    logits, tg = big
    assert tg["obj_mask"].sum() > 0 and np.abs(logits["hm_cen"]).max() < 9
    s = {h: gr.np_sigmoid(logits[h]) for h in SIG}
    preds = probabilities(logits, s)
    got = _host(runtime.LossEvaluator(gpu).grad(_dev(preds, gpu), _dev(tg, gpu)))
    mine = gr.compute_loss_grad(preds, tg)
    for h in HEADS:
        err = np.abs(got[h] - mine[h])
        print(f"loss_grad[152/{h}]: max rel. error {np.max(err / np.maximum(np.abs(mine[h]), 1e-300)):.3e}")
        assert np.all(err <= 1e-6 * np.abs(mine[h])), h
        assert np.all(got[h][mine[h] == 0] == 0)
    got1 = _host(runtime.LossEvaluator(gpu).grad(_dev(logits, gpu), _dev(tg, gpu), apply_sigmoid=True))
    mine1, slack = gr.sigmoid_slack(logits, tg, s)
    for h in HEADS:
        assert np.all(np.abs(got1[h] - mine1[h]) <= 1e-6 * np.abs(mine1[h]) + slack[h]), h


def _bits(d):
    return {k: v.clone().view(torch.int32) for k, v in d.items()}


def test_runs_are_bit_identical_eager_replayed_and_unaligned(gpu):
    logits, tg = _synthetic_case(2, 24, 40, seed=8)
    dl, dt = _dev(logits, gpu), _dev(tg, gpu)
    ev = runtime.LossEvaluator(gpu)
    a = _bits(ev.grad(dl, dt, apply_sigmoid=True))
    b = _bits(ev.grad(dl, dt, apply_sigmoid=True))
    shifted = dict(dl, hm_cen=_offset_view(dl["hm_cen"]), z_coor=_offset_view(dl["z_coor"]))
    c = _bits(ev.grad(shifted, dt, apply_sigmoid=True))
    out = {h: torch.empty_like(dl[h]) for h in HEADS}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.grad(dl, dt, apply_sigmoid=True, verify=False, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.grad(dl, dt, apply_sigmoid=True, verify=False, out=out)
    for t in out.values():
        t.fill_(float("nan"))
    ev.grad_status.fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    for h in HEADS:
        assert not torch.isnan(out[h]).any(), h  # every byte is written by the kernels
        r = out[h].view(torch.int32)
        assert torch.equal(a[h], b[h]) and torch.equal(a[h], c[h]) and torch.equal(a[h], r), h
    assert int(ev.grad_status.item()) == 0
    assert any(bool((v != 0).any()) for v in a.values())


def test_bad_index_raises_index_error(g, gpu):
    logits, tg, _, _ = case_inputs(g, "generic")
    bad = dict(tg, indices_center=tg["indices_center"].copy())
    bad["indices_center"][1, 0] = 64  # == H * W under a set mask bit
    assert bad["obj_mask"][1, 0] == 1
    ev = runtime.LossEvaluator(gpu)
    with pytest.raises(IndexError, match="indices_center"):
        ev.grad(_dev(logits, gpu), _dev(bad, gpu), apply_sigmoid=True)
    bad["indices_center"][1, 0] = -1
    with pytest.raises(IndexError, match="indices_center"):
        ev.grad(_dev(logits, gpu), _dev(bad, gpu))
    bad["obj_mask"] = bad["obj_mask"].copy()
    bad["obj_mask"][1, 0] = 0  # the same slot under a cleared bit is fine
    ev.grad(_dev(logits, gpu), _dev(bad, gpu))
    with pytest.raises(runtime.SfaNativeError, match="GPU"):
        ev.grad({k: torch.from_numpy(v) for k, v in logits.items()}, _dev(tg, gpu))


def test_differentiable_compute_loss_backward(g, gpu):
    from losses.losses import Compute_Loss
    logits, tg, _, _ = case_inputs(g, "dup")
    dt = _dev(tg, gpu)
    want = runtime.LossEvaluator(gpu).grad(_dev(logits, gpu), dt, apply_sigmoid=True)
    ref_total, ref_stats = Compute_Loss(gpu)(_dev(logits, gpu), dt)

    crit = Compute_Loss(gpu, differentiable=True)
    for factor in (1.0, 0.5):
        leaves = {h: v.requires_grad_(True) for h, v in _dev(logits, gpu).items()}
        outputs = dict(leaves)
        total, stats = crit(outputs, dt)
        assert total.dim() == 0 and total.requires_grad and stats == ref_stats
        assert torch.equal(total.detach().view(torch.int32), ref_total.view(torch.int32))
        (total * factor).backward()
        for h in HEADS:
            assert torch.equal(leaves[h].grad.view(torch.int32), (want[h] * factor).view(torch.int32)), (h, factor)
            assert torch.equal(leaves[h].detach(), torch.from_numpy(logits[h]).to(gpu))  # the logits are untouched
        for h in SIG:  # the dict entries hold the clamped sigmoid, detached
            expect = runtime.sigmoid_clamp_(torch.from_numpy(logits[h]).to(gpu))
            assert not outputs[h].requires_grad and torch.equal(outputs[h], expect)
        assert outputs["dim"] is leaves["dim"]

    # behind a torch op: the chain rule reaches a leaf further back; a head that needs no grad gets none
    w = torch.full((), 2.0, device=gpu, requires_grad=True)
    d = _dev(logits, gpu)
    outputs = dict(d, dim=d["dim"] * w)
    total, _ = crit(outputs, dt)
    total.backward()
    gdim = runtime.LossEvaluator(gpu).grad(dict(d, dim=d["dim"] * 2.0), dt, apply_sigmoid=True)["dim"]
    torch.testing.assert_close(w.grad, (gdim * d["dim"]).sum(), rtol=1e-5, atol=1e-6)
    # no input requires grad: the forward still works and total carries no graph
    total, stats = crit(_dev(logits, gpu), dt)
    assert not total.requires_grad and stats == ref_stats
