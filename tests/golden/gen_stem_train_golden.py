"""Writes tests/golden/stem_train_golden.npz: the reference's stem modules (models/fpn_resnet.py:120-123, 179-182:
nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64, momentum=0.1), nn.ReLU, nn.MaxPool2d(3, 2, 1)) in train(),
on the CPU in float32 under torch.autograd, at (B, H, W) = (2, 12, 20) and (1, 6, 10).  The parameters and the running
buffers before the step once; per case x, z, a, pooled, gp, dx (z, a, pooled, gp NHWC; x and dx NCHW), the three
parameter gradients, the running buffers and num_batches_tracked after the step, and ``premises`` = (smallest
|pre-activation|, smallest pool lead, smallest var / mean z^2, smallest distance of a running statistic from the
batch's in batch deviations).  The images are conditioned (stem_train_restatement.condition_image) until the premises
hold, and the generator asserts them on what it stores: pre-activations and pool leads at least MARGIN, the running
statistics at least MIN_FAR batch deviations away, var / mean z^2 at least MIN_COND.  Data only.

    python tests/golden/gen_stem_train_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import golden_io  # noqa: E402
import stem_train_restatement as st  # noqa: E402

CASES = {"b2_12x20": (2, 12, 20, 41), "b1_6x10": (1, 6, 10, 42)}
PARAM_SEED = 3600
MIN_FAR = 1.1
MIN_COND = 0.05


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def reference_stem(p):
    conv = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
    bn = nn.BatchNorm2d(64, momentum=0.1)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(p["conv1"]))
        for t, v in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), p["bn1"]):
            t.copy_(torch.from_numpy(v))
    assert bn.eps == st.EPS and bn.momentum == st.MOMENTUM
    return conv, bn, nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2, padding=1)


def main():
    torch.set_num_threads(1)
    p = st.draw_params(PARAM_SEED)
    out = {"conv1.weight": p["conv1"]}
    for k, v in zip(("weight", "bias", "running_mean", "running_var"), p["bn1"]):
        out[f"bn1.{k}"] = v
    for case, (B, H, W, seed) in CASES.items():
        rng = np.random.default_rng(seed)
        x = st.condition_image(p, rng.standard_normal((B, 3, H, W)).astype(np.float32))
        pre, lead, cond, far = st.premises(x, p)
        assert pre >= st.MARGIN and lead >= st.MARGIN and far >= MIN_FAR and cond >= MIN_COND, (pre, lead, cond, far)
        conv, bn, relu, pool = reference_stem(p)
        conv.train(), bn.train()
        xt = torch.from_numpy(x).requires_grad_()
        z = conv(xt)
        a = relu(bn(z))
        pooled = pool(a)
        psh = tuple(pooled.shape)
        gp = (rng.standard_normal(psh) * (rng.random(psh) < 0.8)).astype(np.float32)
        pooled.backward(torch.from_numpy(gp))
        assert int(bn.num_batches_tracked) == 1
        for k, v in (("x", x), ("z", nhwc(z)), ("a", nhwc(a)), ("pooled", nhwc(pooled)),
                     ("gp", nhwc(torch.from_numpy(gp))), ("dx", xt.grad.numpy()),
                     ("conv1.weight.grad", conv.weight.grad.numpy()), ("bn1.weight.grad", bn.weight.grad.numpy()),
                     ("bn1.bias.grad", bn.bias.grad.numpy()), ("running_mean_after", bn.running_mean.numpy()),
                     ("running_var_after", bn.running_var.numpy())):
            out[f"{case}/{k}"] = np.ascontiguousarray(v, dtype=np.float32)
        out[f"{case}/num_batches_tracked"] = np.array(int(bn.num_batches_tracked))
        out[f"{case}/premises"] = np.array([pre, lead, cond, far])
        print(case, "premises (pre, lead, var / mean z^2, far)", pre, lead, cond, far)
    golden_io.save(HERE, "stem_train_golden", out)
    print(sum(np.asarray(v).nbytes for v in out.values()), "bytes raw")


if __name__ == "__main__":
    main()
