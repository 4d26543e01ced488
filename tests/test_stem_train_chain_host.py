"""The composed gate of the training-mode chain from the image (tests/stem_train_chain.py,
tests/golden/stem_train_chain_golden.npz) on the host: the stored image keeps every pre-activation and stem pool lead
MARGIN from changing, a float32 CPU run of the chain passes the gate, and a stem on running statistics, a dropped
identity skip gradient and a bn1 backward without its sum dY x^ term each miss it by a recorded factor."""
import functools
import os

import numpy as np
import pytest
import torch

import golden_io
import stem_train_chain as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def reference():
    """(fixture, state, the float64 chain's tensors on the stored x, gates, margin)."""
    g = golden_io.load(GOLDEN, "stem_train_chain_golden")
    sd = sc.draw_state()
    o, gr, r, margin = sc.forward_backward(sd, g["x"], want_pre=True)
    return g, sd, sc.tensors(o, gr, r), sc.gates(g), margin


def test_premises_and_gated_tensors():
    g, sd, ref, gate, margin = reference()
    assert g["x"].shape == sc.SHAPE and g["x"].dtype == np.float32
    assert os.path.getsize(os.path.join(GOLDEN, "stem_train_chain_golden.npz")) <= golden_io.MAX_FILE_BYTES
    assert margin >= sc.MARGIN and abs(margin - float(g["margin"])) <= 1e-9
    assert len(ref) == 4 + 61 + 40 and set(gate) == set(ref)
    worst = max(float(v.max()) for v in gate.values())
    print(f"training chain from the image: smallest margin {margin:.3e}, largest gate {worst:.3e}")
    # the step moved every running buffer far beyond its gate
    for k in ref:
        if k.endswith(("running_mean", "running_var")):
            assert float(np.max(sc.metric(sd[k], ref[k]) / gate[k])) > 100, k


def test_float32_run_passes_the_gate():
    g, sd, ref, gate, _ = reference()
    got = sc.tensors(*sc.forward_backward(sd, g["x"], dtype=torch.float32)[:3])
    q, k, _ = sc.worst(got, ref, gate)
    print(f"float32 CPU chain: worst m / gate {q:.3f} ({k})")
    assert q <= 1.0


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_mutants_miss_the_gate(mutant):
    g, sd, ref, gate, _ = reference()
    q, k, _ = sc.worst(sc.tensors(*sc.forward_backward(sd, g["x"], mutant=mutant)[:3]), ref, gate)
    print(f"mutant {mutant}: misses the gate by {q:.4g}x at {k}")
    assert q > 10
