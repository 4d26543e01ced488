#!/usr/bin/env python3
"""Generate tests/golden/headsets_golden.npz by running the REFERENCE's models on head sets other than the
production one.

Same recipe as gen_golden.py / gen_resnet_golden.py (build container only; the reference is imported at run
time from a scratch copy, nothing of it is written here but numbers):

  * models/fpn_resnet.py:296  get_pose_net(18, heads, 64)   sets "one", "five_wide", "eight_full"
  * models/resnet.py:279      get_pose_net(18, heads, 64)   set "five_wide"

(tests/headset_cases.py SETS and FIXTURE_CASES), on the CPU in float32, on the input
hash_uniform(seed, 7, .) of headset_cases.FIXTURE_INPUT, with the weights headset_cases.state_dict_np gives
(synthetic_state_dict over the library's state layout, head biases conditioned; the reference model's own
state_dict names and shapes are asserted equal to that layout, in order).  Contents: per case the head names
in the order the reference's forward emits them and the per-head outputs.  No weights, no code.

Usage:  python tests/golden/gen_headsets_golden.py [--out tests/golden]
"""

from __future__ import annotations

import argparse
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root: oracle/
import gen_golden as gg  # noqa: E402  (the import recipe; puts sfa_hip and tests/ on the path)
import golden_io  # noqa: E402
import headset_cases as hc  # noqa: E402
from sfa_hip import _lib  # noqa: E402


def gen(ref, out):
    import importlib

    import torch
    torch.manual_seed(0)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    x = torch.from_numpy(hc.fixture_input())
    res = {"input_shape_seed": np.array(hc.FIXTURE_INPUT)}
    with torch.no_grad():
        for arch, name in hc.FIXTURE_CASES:
            heads = dict(hc.SETS[name])
            module = importlib.import_module("models.fpn_resnet" if arch == "fpn_resnet_18" else "models.resnet")
            model = gg._quiet(module.get_pose_net, 18, heads, 64, False)
            spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
            assert spec == _lib.state_layout(hc.make_arch(heads, arch)), (arch, name)
            sd = hc.state_dict_np(heads, arch)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            model.eval()
            outs = model(x)
            assert list(outs) == list(heads), (list(outs), list(heads))
            res[f"{arch}/{name}/heads"] = np.array(list(outs))
            for h in heads:
                res[f"{arch}/{name}/{h}"] = outs[h].numpy().copy()
            print(f"{arch} {name}: ok", [float(np.abs(res[f'{arch}/{name}/{h}']).max()) for h in heads])
    golden_io.save(out, "headsets_golden", res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    if not os.path.isdir(gg.REF):
        sys.exit("reference not present: fixtures are generated in the build container only")
    ref = gg._import_reference()
    try:
        gen(ref, a.out)
    finally:
        shutil.rmtree(ref["scratch"], ignore_errors=True)


if __name__ == "__main__":
    main()
