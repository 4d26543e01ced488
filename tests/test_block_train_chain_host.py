"""The composed gate of the batch-statistics chain (tests/block_train_chain.py, tests/golden/block_train_chain_golden.npz)
on the host: the stored input keeps every pre-activation MARGIN from zero, every gate is at most GATE_LIMIT, a float32
CPU run of the chain passes it, and a running-statistics mutant, a wiring mutant (the identity skip's gradient
dropped) and a BatchNorm backward without its sum dY x^ term each miss it by a recorded factor."""
import functools
import os

import numpy as np
import pytest
import torch

import block_train_chain as bc
import golden_io

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def reference():
    """(fixture, state, the float64 chain's tensors on the stored x, gates)."""
    g = golden_io.load(GOLDEN, "block_train_chain_golden")
    sd = bc.draw_state()
    o, gr, r, margin = bc.forward_backward(sd, g["x"], want_pre=True)
    return g, sd, bc.tensors(o, gr, r), bc.gates(g), margin


def test_premises_and_gate_size():
    g, sd, ref, gate, margin = reference()
    assert g["x"].shape == bc.SHAPE and g["x"].dtype == np.float32
    assert margin >= bc.MARGIN and abs(margin - float(g["margin"])) <= 1e-9
    assert len(ref) == 4 + 58 + 38 and set(gate) == set(ref)
    worst = max(float(v.max()) for v in gate.values())
    print(f"batch-statistics chain: smallest |pre-activation| {margin:.3e}, largest gate {worst:.3e}")
    assert worst <= bc.GATE_LIMIT
    # the step moved every running buffer far beyond its gate
    for k in ref:
        if k.endswith(("running_mean", "running_var")):
            assert float(np.max(bc.metric(sd[k], ref[k]) / gate[k])) > 100, k


def test_float32_run_passes_the_gate():
    _, sd, ref, gate, _ = reference()
    got = bc.tensors(*bc.forward_backward(sd, reference()[0]["x"], dtype=torch.float32)[:3])
    q, k, _ = bc.worst(got, ref, gate)
    print(f"float32 CPU chain: worst m / gate {q:.3f} ({k})")
    assert q <= 1.0


@pytest.mark.parametrize("mutant", bc.MUTANTS)
def test_mutants_miss_the_gate(mutant):
    g, sd, ref, gate, _ = reference()
    q, k, _ = bc.worst(bc.tensors(*bc.forward_backward(sd, g["x"], mutant=mutant)[:3]), ref, gate)
    print(f"mutant {mutant}: misses the gate by {q:.4g}x at {k}")
    assert q > 100
