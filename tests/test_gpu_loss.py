"""sfa_compute_loss against the float64 restatement (tests/loss_restatement.py) and the reference's recorded
losses (tests/golden/gen_loss_golden.py).

Bounds.  Against the restatement: relative error <= 1e-6 per component — the focal terms all have one sign
and the L1 terms are non-negative (no cancellation), both sides evaluate in float64 from the same float32
inputs, so what remains is the result's one rounding to float32 (6e-8) and float64 summation order.  Against
the reference: |gpu - ref| <= d_ref + 1e-6 |value|, d_ref = |ref - restatement| recorded in the fixture (the
triangle inequality)."""
import numpy as np
import pytest
import torch

import golden_io
import loss_restatement as lr
from conftest import GOLDEN
from sfa_hip import runtime, synthetic
from test_loss_host import CASES, HEADS, case_loss_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return golden_io.load(GOLDEN, "loss_golden")


def _dev(d, gpu):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu) for k, v in d.items()}


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


@pytest.mark.parametrize("name", CASES)
def test_loss_matches_restatement_and_reference(g, gpu, name):
    preds, tg = case_loss_inputs(g, name)
    ev = runtime.LossEvaluator(gpu)
    got = ev(_dev(preds, gpu), _dev(tg, gpu)).cpu().numpy().astype(np.float64)
    sums = ev.sums.cpu().numpy()
    mine, my_sums = lr.compute_loss(preds, tg)
    ref, d_ref = g[f"{name}/ref_loss"], g[f"{name}/d_ref"]
    print(f"compute_loss[{name}]: gpu {got}\n  rel. vs restatement {_rel(got, mine)}\n  |gpu - ref| {np.abs(got - ref)}"
          f" bound {d_ref + 1e-6 * np.abs(ref)}")
    assert np.all(np.abs(got - mine) <= 1e-6 * np.abs(mine)), (got, mine)
    assert np.all(np.abs(got - ref) <= d_ref + 1e-6 * np.abs(ref)), (got, ref)
    assert sums[2] == my_sums[2] and sums[7] == my_sums[7]  # num_pos, mask sum: exact counts
    # float64 sums of like-signed terms: at most n = 2304 cells x 1.1e-16 of order-dependent rounding plus a
    # few ulp of log per term, under 3e-13 relative
    assert np.all(np.abs(sums - my_sums) <= 1e-12 * np.abs(my_sums))
    assert int(ev.status.item()) == 0


def _synthetic_case(B, H, W, C=3, M=50, seed=3):
    labels, offsets = synthetic.synthetic_labels(B, seed=seed)
    tg, _ = lr.build_targets_batch(labels, offsets, [b % 2 == 1 for b in range(B)], hm_size=(H, W), num_classes=C,
                                   max_objects=M)
    preds = {h: synthetic.synthetic_logits((B, c, H, W), seed, 40 + i, 2.0)
             for i, (h, c) in enumerate(zip(HEADS, (C, 2, 2, 1, 3)))}
    return preds, tg


@pytest.mark.parametrize("shape", [(4, 152, 152), (1, 5, 7)])
def test_synthetic_shapes_match_the_restatement(gpu, shape):
    """152 x 152, B = 4: 68 focal blocks (the fixture maps take 1), the production shape.  5 x 7, B = 1:
    105 cells, not a multiple of the 4-wide loads."""
    B, H, W = shape
    preds, tg = _synthetic_case(B, H, W)
    assert tg["obj_mask"].sum() > 0
    ev = runtime.LossEvaluator(gpu)
    dp = _dev(preds, gpu)
    got = ev(dp, _dev(tg, gpu), apply_sigmoid=True).cpu().numpy().astype(np.float64)
    # the restatement on the GPU's own clamped probabilities (its expf is not numpy's, bit for bit)
    probs = dict(preds)
    for h in ("hm_cen", "cen_offset"):
        probs[h] = runtime.sigmoid_clamp_(dp[h].clone()).cpu().numpy()
    mine, _ = lr.compute_loss(probs, tg)
    print(f"compute_loss[{shape}]: rel. vs restatement {_rel(got, mine)}")
    assert np.all(np.abs(got - mine) <= 1e-6 * np.abs(mine)), (got, mine)


@pytest.mark.parametrize("name", ["misc2432", "borders16"])
def test_apply_sigmoid_is_bit_identical_to_the_in_place_kernel(g, gpu, name):
    logits = {h: g[f"{name}/logits/{h}"] for h in HEADS}
    _, tg = case_loss_inputs(g, name)
    ev = runtime.LossEvaluator(gpu)
    d_tg = _dev(tg, gpu)
    fused = ev(_dev(logits, gpu), d_tg, apply_sigmoid=True).clone()
    fused_sums = ev.sums.clone()
    pre = _dev(logits, gpu)
    runtime.sigmoid_clamp_(pre["hm_cen"])
    runtime.sigmoid_clamp_(pre["cen_offset"])
    split = ev(pre, d_tg, apply_sigmoid=False)
    assert torch.equal(fused.view(torch.int32), split.view(torch.int32))
    assert torch.equal(fused_sums.view(torch.int64), ev.sums.view(torch.int64))


def test_runs_are_bit_identical_and_alignment_free(gpu):
    """Two runs give the same bits; a heat map that is not 16-byte aligned (scalar loads) gives the bits of
    the aligned one (128-bit loads): the partition and the order of the sums are the same."""
    preds, tg = _synthetic_case(2, 24, 40, seed=8)
    dp, dt = _dev(preds, gpu), _dev(tg, gpu)
    ev = runtime.LossEvaluator(gpu)
    a, sa = ev(dp, dt, apply_sigmoid=True).clone(), ev.sums.clone()
    b, sb = ev(dp, dt, apply_sigmoid=True).clone(), ev.sums.clone()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(sa.view(torch.int64), sb.view(torch.int64))
    n = dp["hm_cen"].numel()
    shifted = torch.empty(n + 1, dtype=torch.float32, device=gpu)[1:].view(dp["hm_cen"].shape)
    shifted.copy_(dp["hm_cen"])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    dp2 = dict(dp, hm_cen=shifted)
    c = ev(dp2, dt, apply_sigmoid=True)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and torch.equal(sa.view(torch.int64), ev.sums.view(torch.int64))


def test_graph_replay_equals_eager(g, gpu):
    preds, tg = case_loss_inputs(g, "misc2432")
    dp, dt = _dev(preds, gpu), _dev(tg, gpu)
    ev = runtime.LossEvaluator(gpu)
    eager, eager_sums = ev(dp, dt).clone(), ev.sums.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev(dp, dt, verify=False)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev(dp, dt, verify=False)
    ev.loss.fill_(-1)
    ev.sums.fill_(-1)
    ev.status.fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ev.loss.view(torch.int32), eager.view(torch.int32))
    assert torch.equal(ev.sums.view(torch.int64), eager_sums.view(torch.int64)) and int(ev.status.item()) == 0


def test_bad_index_raises_index_error(g, gpu):
    """An index >= H*W under a set mask bit: the reference's gather raises; here the slot adds nothing, the
    status word says so and Compute_Loss raises IndexError."""
    from losses.losses import Compute_Loss
    logits = {h: g[f"outmap2432/logits/{h}"] for h in HEADS}
    tg = {k: g[f"outmap2432/t/{k}"] for k in lr.KEYS}  # as build_targets gave them: slot (0, 1) is past the map
    assert (tg["indices_center"][tg["obj_mask"] == 1] >= 24 * 32).any()
    crit = Compute_Loss(gpu)
    with pytest.raises(IndexError, match="indices_center"):
        crit(_dev(logits, gpu), _dev(tg, gpu))
    # the same slot under a cleared mask bit is fine, as in the reference
    _, ok = case_loss_inputs(g, "outmap2432")
    outputs = _dev(logits, gpu)
    total, stats = crit(outputs, _dev(ok, gpu))
    assert total.dim() == 0 and total.device.type == "cuda" and list(stats) == list(lr.LOSS_KEYS)
    # outputs hold the clamped sigmoid afterwards (losses.py:140-141); the restatement on those probabilities
    probs = {h: outputs[h].cpu().numpy() for h in HEADS}
    assert probs["hm_cen"].min() >= np.float32(1e-4) and probs["hm_cen"].max() <= np.float32(1 - 1e-4)
    mine, _ = lr.compute_loss(probs, ok)
    got = np.array([stats[k] for k in lr.LOSS_KEYS])
    assert np.all(np.abs(got - mine) <= 1e-6 * np.abs(mine)), (got, mine)
    assert float(total) == stats["total_loss"]
