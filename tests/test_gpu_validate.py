"""The validation tier end to end through the reference's module paths: create_model -> forward ->
TargetBuilder -> losses.losses.Compute_Loss, for both detector families, against the float64 restatement fed
the GPU's own head maps (bound: tests/test_gpu_loss.py, 1e-6 relative per component)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import loss_restatement as lr
from conftest import REPO
from sfa_hip import runtime, synthetic

pytestmark = pytest.mark.gpu


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _model(arch, gpu):
    from models.model_utils import create_model
    model = create_model(Cfg(arch=arch, heads=dict(runtime.DEFAULT_HEADS), head_conv=64, imagenet_pretrained=False))
    spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    sd = synthetic.synthetic_state_dict(spec, 0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(gpu).eval()


@pytest.mark.parametrize("arch", ["fpn_resnet_18", "resnet_18"])
def test_validation_step(gpu, arch):
    from losses.losses import Compute_Loss  # the reference's import line, served by the drop-in tree
    model = _model(arch, gpu)
    x = torch.from_numpy(synthetic.synthetic_bev(2, 96, 96, seed=3)).to(gpu)
    labels, offsets = synthetic.synthetic_labels(2, seed=4)
    builder = runtime.TargetBuilder(gpu, runtime.DEFAULT_BOUNDARY, (24, 24), 3, 50)
    targets = builder(labels, offsets.tolist(), [False, True])
    assert int(targets["obj_mask"].sum()) > 0
    with torch.no_grad():
        outputs = model(x)
    logits = {h: outputs[h].clone() for h in outputs}
    total, stats = Compute_Loss(gpu)(outputs, targets)
    assert list(stats) == list(lr.LOSS_KEYS) and all(isinstance(v, float) for v in stats.values())
    assert total.dim() == 0 and total.device == gpu and float(total) == stats["total_loss"]
    parts = np.float64([stats[k] for k in lr.LOSS_KEYS[1:]])
    # total and parts are roundings of the same float64 values: half an ulp each of six float32 numbers
    assert abs(stats["total_loss"] - parts.sum()) <= 6 * 2.0 ** -24 * max(abs(stats["total_loss"]), np.abs(parts).max())
    # outputs now hold the clamped sigmoid (losses.py:140-141), the other heads are untouched
    for h in ("hm_cen", "cen_offset"):
        assert torch.equal(outputs[h], runtime.sigmoid_clamp_(logits[h].clone()))
    assert torch.equal(outputs["dim"], logits["dim"])
    preds = {h: outputs[h].cpu().numpy() for h in outputs}
    mine, _ = lr.compute_loss(preds, {k: v.cpu().numpy() for k, v in targets.items()})
    got = np.float64([stats[k] for k in lr.LOSS_KEYS])
    print(f"validate[{arch}]: loss {got}, rel. vs restatement {np.abs(got - mine) / np.abs(mine)}")
    assert np.all(np.abs(got - mine) <= 1e-6 * np.abs(mine)), (got, mine)
    # and the targets are the restatement's
    ref, _ = lr.build_targets_batch(labels, offsets, [False, True], hm_size=(24, 24), num_classes=3, max_objects=50)
    np.testing.assert_array_equal(targets["indices_center"].cpu().numpy(), ref["indices_center"])
    np.testing.assert_array_equal(targets["obj_mask"].cpu().numpy(), ref["obj_mask"])


def test_validate_tool_synthetic(gpu, capsys):
    """tools/validate.py --synthetic: one JSON line with the averaged loss (in process: no second GPU client)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import validate
    finally:
        sys.path.pop(0)
    res = validate.main(["--synthetic", "3", "--batch_size", "2", "--input_size", "96"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    assert json.loads(line)["val_loss"] == res["val_loss"]
    assert res["frames"] == 3 and np.isfinite(res["val_loss"]) and res["val_loss"] > 0
    assert set(res["loss_stats"]) == set(lr.LOSS_KEYS)
