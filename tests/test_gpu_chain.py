"""The composed training chain on the GPU against the float64 restatement of the whole network
(tests/chain_restatement.py): PoseResNet.detect_from_pooled, detect_from_layers, neck_trainable() and
heads_trainable(), each through Compute_Loss(differentiable=True) and backward(), at the two cases of
chain_restatement.CASES.  Every gradient is held to gate(t) = 4 (noise32(t) + perturb(t)) in both forms of
chain_restatement.metric; the gate was measured on the CPU (tests/golden/gen_chain_golden.py) and is at most 1e-2
(tests/test_chain_host.py), where a wiring mistake moves a gradient by tens of percent.
Each test prints its worst m / gate per parameter group; DESIGN.md section 28 records them."""
import functools

import numpy as np
import pytest
import torch

import chain_restatement as cr
import loss_restatement as lr
from sfa_hip import runtime
from test_chain_host import CASES, LAYERS, case_reference, model_state

pytestmark = pytest.mark.gpu
STEM = set(cr.STEM)


@pytest.fixture(autouse=True)
def _grad_mode():
    """Autograd on whatever an earlier test module left the process-wide switch at."""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def model(gpu):
    from models.fpn_resnet import get_pose_net
    m = get_pose_net(18, dict(runtime.DEFAULT_HEADS), 64, False)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in model_state().items()})
    return m.to(gpu).eval()


@functools.lru_cache(maxsize=None)
def cut_reference(case, cut):
    """The float64 restatement behind the float32 rounding of its own pooled map ("pooled") or backbone maps
    ("layers"): the very numbers the GPU is given as leaves."""
    r = case_reference(case)
    if cut == "pooled":
        inp = r["inter"]["pooled"].astype(np.float32)
    else:
        inp = [r["inter"][n].astype(np.float32) for n in LAYERS]
    loss, maps, grads = cr.forward_backward(model_state(), inp, r["inputs"]["targets"])
    return dict(inp=inp, loss=loss, maps=maps, grads=grads)


def _targets(gpu, case):
    """TargetBuilder's targets of the case's labels; they are the restatement's, bit for bit."""
    c, inp = cr.CASES[case], case_reference(case)["inputs"]
    tg = runtime.TargetBuilder(gpu, hm_size=(c["H"] // 4, c["W"] // 4))(inp["labels"], inp["offsets"])
    for k, v in inp["targets"].items():
        assert np.array_equal(tg[k].cpu().numpy(), v), k
    return tg


def _loss_backward(gpu, case, outs):
    """Compute_Loss(differentiable=True) and backward(); the loss terms against loss_restatement.compute_loss on the
    GPU's own maps and clamped sigmoids, to the loss test's 1e-6 (tests/test_gpu_loss.py)."""
    from losses.losses import Compute_Loss
    assert list(outs) == list(runtime.DEFAULT_HEADS)
    maps = {k: v.detach().clone() for k, v in outs.items()}
    total, stats = Compute_Loss(gpu, differentiable=True)(dict(outs), _targets(gpu, case))
    total.backward()
    torch.cuda.synchronize()
    probs = {k: v.cpu().numpy() for k, v in maps.items()}
    for h in ("hm_cen", "cen_offset"):
        probs[h] = runtime.sigmoid_clamp_(maps[h].clone()).cpu().numpy()
    mine, _ = lr.compute_loss(probs, case_reference(case)["inputs"]["targets"])
    got = np.array([stats[k] for k in lr.LOSS_KEYS])
    assert np.all(np.abs(got - mine) <= 1e-6 * np.abs(mine)), (got, mine)
    return {k: v.cpu().numpy() for k, v in maps.items()}, got


def _hold(label, got, ref, gate, rename=None):
    """Every tensor of ``got`` at its gate, both forms; prints the worst m / gate per group."""
    rename = rename or {}
    gates = {k: gate[rename.get(k, k)] for k in got}
    worst = cr.worst_ratios(got, ref, gates, list(got))
    print(f"{label}: worst m / gate " + "  ".join(f"{grp} {q:.3f} ({k})" for grp, (q, k) in sorted(worst.items())))
    bad = {grp: v for grp, v in worst.items() if not v[0] <= 1.0}
    assert not bad, bad


def _param_grads(model, expect):
    named = dict(model.named_parameters())
    assert len(named) == 126
    reached = {k for k, p in named.items() if p.grad is not None}
    assert reached == expect, sorted(reached ^ expect)
    return {k: named[k].grad.cpu().numpy() for k in sorted(reached)}


def _zero(model):
    for p in model.parameters():
        p.grad = None


@pytest.mark.parametrize("case", CASES)
def test_detect_from_pooled(gpu, model, case):
    r, ref = case_reference(case), cut_reference(case, "pooled")
    _zero(model)
    x = torch.from_numpy(ref["inp"]).to(gpu).requires_grad_()
    maps, loss = _loss_backward(gpu, case, model.detect_from_pooled(x))
    got = _param_grads(model, set(dict(model.named_parameters())) - STEM)
    assert len(got) == 123
    got["x"] = x.grad.cpu().numpy()
    _hold(f"detect_from_pooled[{case}]", got, ref["grads"], r["gate"], {"x": "pooled"})
    # the five maps at the composed forward gate.  Carrying 1e-5 max(1, |v|) per stage through the |W'| sums of the 22
    # convolution stages behind the pooled map, as the two-block test does over four, gives a bound above any float64
    # (row sums of |W'| are 20 to 50 per stage), so the composed gate is the measured one: the same 4 (noise32 +
    # perturb), where perturb is that per-stage deviation drawn at random in the float64 restatement.
    for h in cr.HEADS:
        m = cr.metric(maps[h], ref["maps"][h]) / r["gate"][f"map/{h}"]
        print(f"  map {h}: m / gate {m.max():.3f}")
        assert np.all(m <= 1.0), h
    assert np.all(np.abs(loss - ref["loss"]) <= 1e-3 * np.abs(ref["loss"]))  # the same loss, not another one


@pytest.mark.parametrize("case", CASES)
def test_detect_from_layers(gpu, model, case):
    r, ref = case_reference(case), cut_reference(case, "layers")
    _zero(model)
    leaves = [torch.from_numpy(a).to(gpu).requires_grad_() for a in ref["inp"]]
    _loss_backward(gpu, case, model.detect_from_layers(*leaves))
    got = _param_grads(model, {k for k in dict(model.named_parameters()) if cr.group_of(k) in ("neck", "heads")})
    assert len(got) == 66
    got.update({n: t.grad.cpu().numpy() for n, t in zip(LAYERS, leaves)})
    _hold(f"detect_from_layers[{case}]", got, ref["grads"], r["gate"])


@pytest.mark.parametrize("mode,groups", [("neck_trainable", ("neck", "heads")), ("heads_trainable", ("heads",))])
@pytest.mark.parametrize("case", CASES)
def test_trainable_modes_from_the_image(gpu, model, case, mode, groups):
    r = case_reference(case)
    _zero(model)
    x = torch.from_numpy(r["inputs"]["image"]).to(gpu).requires_grad_()
    getattr(model, mode)()
    try:
        _loss_backward(gpu, case, model(x))
    finally:
        getattr(model, mode)(False)
    got = _param_grads(model, {k for k in dict(model.named_parameters()) if cr.group_of(k) in groups})
    assert len(got) == (66 if "neck" in groups else 60) and x.grad is None
    _hold(f"{mode}[{case}]", got, r["grads"], r["gate"])


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_accumulation_and_repetition_are_bit_exact(gpu, model):
    case = "c1_32x160"
    ref = cut_reference(case, "pooled")
    x = torch.from_numpy(ref["inp"]).to(gpu).requires_grad_()
    params = [p for k, p in model.named_parameters() if k not in STEM]

    def run():
        _loss_backward(gpu, case, model.detect_from_pooled(x))
        return [t.grad.clone() for t in [x] + params]

    _zero(model)
    x.grad = None
    first = run()
    twice = run()  # nothing zeroed: .grad accumulates
    assert all(_bits(b, 2 * a) for a, b in zip(first, twice))
    _zero(model)
    x.grad = None
    again = run()
    assert all(_bits(a, b) for a, b in zip(first, again))
