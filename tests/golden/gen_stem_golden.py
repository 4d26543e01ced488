"""Writes tests/golden/stem_golden.npz: the reference's stem (models/fpn_resnet.py:179-182: nn.Conv2d(3, 64, 7, 2, 3,
bias=False), nn.BatchNorm2d(64), nn.ReLU, nn.MaxPool2d(3, 2, 1)) in eval() with drawn running statistics, on the CPU in
float32 under torch.autograd, at (B, H, W) = (2, 12, 20) and (1, 6, 10).  Per case: x, a, pooled, gp, dx and the
gradients of conv1.weight, bn1.weight, bn1.bias, all stored in full (NCHW, as torch has them); the parameters once.
The images are conditioned (stem_restatement.condition_image) so that every pre-activation and every pooling
window's lead stays MARGIN away from changing; the generator asserts it on what it stores.  Data only.

    python tests/golden/gen_stem_golden.py
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
import stem_restatement as sr  # noqa: E402

CASES = {"b2_12x20": (2, 12, 20, 31), "b1_6x10": (1, 6, 10, 32)}
PARAM_SEED = 2900


def reference_stem(p):
    conv = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
    bn = nn.BatchNorm2d(64, momentum=0.1)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(p["conv1"]))
        for t, v in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), p["bn1"]):
            t.copy_(torch.from_numpy(v))
    return conv, bn, nn.Sequential(conv, bn, nn.ReLU(inplace=True)).eval(), nn.MaxPool2d(kernel_size=3, stride=2, padding=1)


def main():
    torch.set_num_threads(1)
    p = sr.draw_params(PARAM_SEED)
    out = {"conv1.weight": p["conv1"]}
    for k, v in zip(("weight", "bias", "running_mean", "running_var"), p["bn1"]):
        out[f"bn1.{k}"] = v
    for case, (B, H, W, seed) in CASES.items():
        rng = np.random.default_rng(seed)
        x = sr.condition_image(p, rng.standard_normal((B, 3, H, W)).astype(np.float32))
        assert sr.margins(p, x) >= sr.MARGIN
        conv, bn, front, pool = reference_stem(p)
        xt = torch.from_numpy(x).requires_grad_()
        a = front(xt)
        a.retain_grad()
        pooled = pool(a)
        gp = (rng.standard_normal(tuple(pooled.shape)) * (rng.random(tuple(pooled.shape)) < 0.8)).astype(np.float32)
        pooled.backward(torch.from_numpy(gp))
        for k, v in (("x", x), ("a", a.detach().numpy()), ("pooled", pooled.detach().numpy()), ("gp", gp),
                     ("dx", xt.grad.numpy()), ("conv1.weight.grad", conv.weight.grad.numpy()),
                     ("bn1.weight.grad", bn.weight.grad.numpy()), ("bn1.bias.grad", bn.bias.grad.numpy())):
            out[f"{case}/{k}"] = np.ascontiguousarray(v, dtype=np.float32)
        print(case, "margin", sr.margins(p, x))
    golden_io.save(HERE, "stem_golden", out)
    print(sum(v.nbytes for v in out.values()), "bytes raw")


if __name__ == "__main__":
    main()
