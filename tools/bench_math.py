"""bench.py with the opt-in reduced-precision mode added to its tables.

    python tools/bench_math.py --math fp16 [any bench.py argument]

bench.py's own --math lists the three parity-class modes only (and SFA_MATH=fp16 fails at its name lookup).
This wrapper adds an `fp16` entry to bench.MATHS / PEAKS / PEAKS_CAPPED / DTYPES at run time and calls
bench.main() with the caller's arguments, so SFA_MATH_FP16 (include/sfa_hip.h) is timed by the same harness
and prints the same JSON line.  Peak: dense fp16 MFMA, one product per MAC.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402
from sfa_hip import _lib  # noqa: E402  (bench put the package on sys.path)

bench.MATHS["fp16"] = _lib.MATH_FP16
bench.PEAKS["fp16"] = (bench.PEAK_BF16_MFMA_TFLOPS, "dense fp16 MFMA 2500 TF, one fp16 product per MAC")
bench.PEAKS_CAPPED["fp16"] = bench.MEASURED_FP16_MFMA_CAPPED_TFLOPS
bench.DTYPES["fp16"] = ("f32 tensors (fp16: power-of-two-scaled operands rounded once to fp16, 1 product, "
                        "f32 accumulate; stem and FPN fp16x3) — below the 1e-5 parity class")

_roofline_line = bench.roofline_line


def roofline_line(args, *a, **kw):
    """bench.roofline_line names the heads kernel per mode from its own table: the fp16x3 row with the kernel
    name and the traffic corrected (the committed PMC passes measured the fp16x3 kernels, not these)."""
    if args.math != "fp16":
        return _roofline_line(args, *a, **kw)
    import copy
    as_x3 = copy.copy(args)
    as_x3.math = "fp16x3"
    line = _roofline_line(as_x3, *a, **kw)
    if "conv_r3_kernel" in str(line.get("kernel", "")):
        line["kernel"] = ("conv_r3_kernel<256, 320, ..., TERMS = 1> (fused detection heads, one fp16 product per "
                          "MAC; one launch per KFPN level)")
    else:
        line["kernel"] = "the whole forward (math fp16)"
    line["traffic"] = None
    line["traffic_basis"] = "null: no PMC pass of the fp16 mode's kernels is committed"
    if isinstance(line.get("forward"), dict):
        line["forward"]["traffic"] = None
    return line


bench.roofline_line = roofline_line

if __name__ == "__main__":
    bench.main()
