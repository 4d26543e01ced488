#!/usr/bin/env python3
"""The composed gate of the training-mode chain from the image (stem_from_image + layers_from_pooled, both with
batch_stats=True), measured on the CPU (tests/stem_train_chain.py).

A seeded (2, 3, 64, 96) image is conditioned until every pre-activation and every stem pool window's lead of the
float64 chain lies at least MARGIN from changing; then, per gated tensor t (out_layer1..4, the gradients at x and the
60 stem and block parameters, the 40 running buffers after the step), in both forms of chain_restatement.metric:
  noise32/<t>   the float32 CPU run of the same chain against the float64 one
  perturb/<t>   the float64 chain with every stage moved by GATE max(1, |v|) U(-1, 1) against the unmoved one
Output: tests/golden/stem_train_chain_golden.npz (data only): x (f32), margin, the two families, ``torch_version``."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import golden_io  # noqa: E402
import stem_train_chain as sc  # noqa: E402


def main():
    torch.set_num_threads(8)
    sd = sc.draw_state()
    x = sc.condition_image(sd, np.random.default_rng(4200).standard_normal(sc.SHAPE))
    o, g, r, margin = sc.forward_backward(sd, x, want_pre=True)
    ref = sc.tensors(o, g, r)
    f32 = sc.tensors(*sc.forward_backward(sd, x, dtype=torch.float32)[:3])
    per = sc.tensors(*sc.forward_backward(sd, x, perturb=np.random.default_rng(4201))[:3])
    out = {"x": x, "margin": np.array(margin), "torch_version": np.array(torch.__version__)}
    for k in ref:
        out["noise32/" + k] = sc.metric(f32[k], ref[k])
        out["perturb/" + k] = sc.metric(per[k], ref[k])
    golden_io.save(HERE, "stem_train_chain_golden", out)
    gate = {k: sc.GATE_FACTOR * (out["noise32/" + k] + out["perturb/" + k]) for k in ref}
    print("margin", margin, "largest gate", max(float(v.max()) for v in gate.values()))
    for m in sc.MUTANTS:
        q, k, _ = sc.worst(sc.tensors(*sc.forward_backward(sd, x, mutant=m)[:3]), ref, gate)
        print("mutant", m, "misses by", q, "at", k)


if __name__ == "__main__":
    main()
