#!/usr/bin/env python3
"""The composed gate of layers_from_pooled(x, batch_stats=True), measured on the CPU (tests/block_train_chain.py).

A seeded (2, 64, 16, 24) input is conditioned until every pre-activation of the float64 chain lies at least MARGIN
from zero; then, per gated tensor t (out_layer1..4, the gradients at x and the 57 parameters, the 38 running buffers
after the step), in both forms of chain_restatement.metric:
  noise32/<t>   the float32 CPU run of the same chain against the float64 one
  perturb/<t>   the float64 chain with every stage moved by GATE max(1, |v|) U(-1, 1) against the unmoved one
Output: tests/golden/block_train_chain_golden.npz (data only): x (f32), margin, the two families, ``torch_version``."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import block_train_chain as bc  # noqa: E402
import golden_io  # noqa: E402


def main():
    torch.set_num_threads(8)
    sd = bc.draw_state()
    x = bc.condition_input(sd, np.random.default_rng(4000).standard_normal(bc.SHAPE))
    o, g, r, margin = bc.forward_backward(sd, x, want_pre=True)
    ref = bc.tensors(o, g, r)
    f32 = bc.tensors(*bc.forward_backward(sd, x, dtype=torch.float32)[:3])
    per = bc.tensors(*bc.forward_backward(sd, x, perturb=np.random.default_rng(4001))[:3])
    out = {"x": x, "margin": np.array(margin), "torch_version": np.array(torch.__version__)}
    for k in ref:
        out["noise32/" + k] = bc.metric(f32[k], ref[k])
        out["perturb/" + k] = bc.metric(per[k], ref[k])
    golden_io.save(HERE, "block_train_chain_golden", out)
    gate = {k: bc.GATE_FACTOR * (out["noise32/" + k] + out["perturb/" + k]) for k in ref}
    print("margin", margin, "largest gate", max(float(v.max()) for v in gate.values()))
    for m in bc.MUTANTS:
        q, k, _ = bc.worst(bc.tensors(*bc.forward_backward(sd, x, mutant=m)[:3]), ref, gate)
        print("mutant", m, "misses by", q, "at", k)


if __name__ == "__main__":
    main()
