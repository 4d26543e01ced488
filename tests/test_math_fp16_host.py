"""SFA_MATH_FP16 (opt-in one-product fp16 mode) — host side: the ABI value, the Python names, and the CPU
emulation (tests/fp16_emulation.py) that sets the mode's tolerances (profiles/fp16_error_budget.json)."""
import json
import os
import re

import numpy as np
import pytest
import torch

import fp16_emulation as emu
import golden_cases as gc
from sfa_hip import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_fp16():
    with open(os.path.join(REPO, "include", "sfa_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"enum\s+sfa_math\s*\{([^}]*)\}", hdr)
    assert m, "enum sfa_math"
    vals = dict(re.findall(r"(SFA_MATH_\w+)\s*=\s*(\d+)", m.group(1)))
    assert vals == {"SFA_MATH_F32": "0", "SFA_MATH_BF16X6": "1", "SFA_MATH_FP16X3": "2", "SFA_MATH_FP16": "3"}


def test_lib_constant():
    assert _lib.MATH_FP16 == 3
    assert (_lib.MATH_F32, _lib.MATH_BF16X6, _lib.MATH_FP16X3) == (0, 1, 2)


def test_math_from_env(monkeypatch):
    monkeypatch.setenv("SFA_MATH", "fp16")
    assert _lib.math_from_env() == _lib.MATH_FP16
    monkeypatch.setenv("SFA_MATH", "fp16x3")
    assert _lib.math_from_env() == _lib.MATH_FP16X3
    monkeypatch.setenv("SFA_MATH", "fp17")
    with pytest.raises(ValueError) as ei:
        _lib.math_from_env()
    for name in ("f32", "bf16x6", "fp16x3", "'fp16'"):
        assert name in str(ei.value), (name, str(ei.value))


@pytest.fixture(scope="module")
def small_errors(golden):
    """{case: {terms: {head: max |emu - ref| / max(1, |ref|)}}} — computed once for the tests below."""
    sd = {k: torch.from_numpy(v) for k, v in gc.state_dict_np(golden.model).items()}
    res = {}
    for case in gc.MODEL_CASES:
        x = torch.from_numpy(gc.model_input(case))
        res[case] = {}
        for terms in (1, 2):
            out = emu.forward(sd, x, gc.HEADS, terms)
            res[case][terms] = {h: emu.rel_err(out[h], golden.model[f"{case}/{h}"]) for h in gc.HEADS}
    return res


@pytest.mark.parametrize("case", list(gc.MODEL_CASES))
def test_emulation_terms2_reproduces_reference(small_errors, case):
    """At two terms (fp16x3) the emulation is f32-class: the project's per-kernel gate."""
    for h, e in small_errors[case][2].items():
        print(f"{case} {h}: terms 2 err {e:.3g}")
        assert e <= 1e-5, (h, e)


@pytest.mark.parametrize("case", list(gc.MODEL_CASES))
def test_emulation_terms1_equals_committed_budget(small_errors, case):
    """The committed budget is what the emulation gives (f64 accumulation: deterministic), to 3 digits."""
    with open(os.path.join(REPO, "profiles", "fp16_error_budget.json")) as f:
        budget = json.load(f)["cases"][case]["fp16"]
    for h, e in small_errors[case][1].items():
        print(f"{case} {h}: terms 1 err {e:.3g} (budget {budget[h]:.3g})")
        assert float(f"{e:.3g}") == pytest.approx(budget[h], rel=1e-12), (h, e, budget[h])


@pytest.mark.parametrize("case", list(gc.MODEL_CASES))
def test_emulation_terms1_less_accurate(small_errors, case):
    for h in gc.HEADS:
        assert small_errors[case][1][h] > small_errors[case][2][h], h


def test_round_terms_is_the_fp16x3_high_term():
    """terms = 1 keeps exactly the hi of the two-term split (one rounding to nearest even)."""
    v = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 12345.678, -0.3333333, 2.0 ** -20], dtype=torch.float64)
    hi1, lo1 = emu.round_terms(v, 1)
    hi2, lo2 = emu.round_terms(v, 2)
    assert lo1 is None and torch.equal(hi1, hi2)
    assert hi1[0].item() == 1.0 and hi1[1].item() == 1.0 + 2.0 ** -9  # ties to even
    assert float(np.max(np.abs((hi2 + lo2 - v).numpy() / v.numpy()))) < 2.0 ** -21
