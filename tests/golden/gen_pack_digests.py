#!/usr/bin/env python3
"""Generate tests/golden/pack_digests.json: the SHA-256 of the input state bytes and of the bytes sfa_pack_weights(_ex)
writes for them, for every case of tests/pack_cases.digest_cases (the edge state of each whole-model case of
tests/test_gpu_pack.py, and synthetic_state_dict for two seeds over every head set of tests/headset_cases.py in both
families).

The file pins the packed bytes across refactors of the pack: run this with the library built at the commit whose
bytes are to be kept (the file records it), never with the code a change is about to be judged by.  The host pack
touches no device, so no GPU is needed.  The states come from a counter hash (sfa_hip/synthetic.py) and are the same
on every machine; the state digest is there to show that.

Usage:  python tests/golden/gen_pack_digests.py [--out tests/golden]
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "lidar-image_object-detection_-fpn_resnet-yolov8_amd", "sfa"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import pack_cases  # noqa: E402


def _git(*args):
    return subprocess.run(["git", "-C", REPO] + list(args), capture_output=True, text=True, check=True).stdout.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    if _git("status", "--porcelain", "--", "lidar-image_object-detection_-fpn_resnet-yolov8_amd/csrc", "include"):
        sys.exit("csrc/ or include/ differs from the commit: the digests must come from a committed pack")
    cases = {}
    for cid, (arch, state) in pack_cases.digest_cases().items():
        s, p = pack_cases.digests(arch, state())
        cases[cid] = {"state_sha256": s, "packed_sha256": p}
        print(cid, s[:12], p[:12])
    doc = {"commit": _git("rev-parse", "HEAD"), "what": "sha256 of the float32 state bytes in layout order and of the "
           "packed buffer sfa_pack_weights(_ex) writes for them", "cases": cases}
    with open(os.path.join(a.out, "pack_digests.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
