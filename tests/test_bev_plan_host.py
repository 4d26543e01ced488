"""The host-only plan checks, built with ASan + UBSan and run as stand-alone programs:
tools/bev_plan_check.cpp (csrc/bev_plan.h: the voxelisers' paths and scratch regions),
tools/decode_plan_check.cpp (csrc/decode_plan.h: tile plans and workspace layouts) and
tools/conv_plan_check.cpp (csrc/conv_args.h, csrc/conv_plan.h: the conv launchers' checks, the stem's
frame chunks, the dispatch predicates).  CPU only: the headers are plain C++, so no program needs HIP
or a GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,expect", [("bev_plan_check", " plans, 0 bad"), ("decode_plan_check", " 0 bad"),
                                         ("conv_plan_check", " checks, 0 bad")])
def test_plan_check_under_host_sanitizers(tmp_path, name, expect):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / name)
    cmd = [gxx, "-std=c++17", "-g", "-O2", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", name + ".cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0"))
    assert r.returncode == 0 and expect in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
