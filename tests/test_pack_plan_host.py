"""The weight-pack plan on the host (csrc/pack_plan.h): tools/pack_plan_check.cpp, built with ASan + UBSan and
run as a stand-alone program over both families and every head set of headset_cases.py; the host pack itself
(csrc/pack_host.h, csrc/pack_row.h): tools/pack_host_check.cpp, built the same way with the ROCm clang++, over the
head sets of pack_cases.CASES; and the ABI of the device pack (include/sfa_hip.h sfa_pack_weights_device(_ex)).
CPU only: the headers include no HIP."""
import ctypes
import os
import shutil
import subprocess

import pytest

import headset_cases as hc
import pack_cases
from sfa_hip import _lib, runtime

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -2  # include/sfa_hip.h sfa_status


def _set_arg(heads):
    return ",".join(f"{k}:{v}" for k, v in heads.items())


def test_pack_plan_check_under_host_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "pack_plan_check")
    cmd = [gxx, "-std=c++17", "-g", "-O2", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(REPO, "tools", "pack_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    sets = [_set_arg(runtime.DEFAULT_HEADS)] + [_set_arg(h) for h in hc.SETS.values()]
    r = subprocess.run([exe] + sets, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0"))
    assert r.returncode == 0 and f"{len(sets)} head sets, " in r.stdout and " checks, 0 bad" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_host_pack_under_host_sanitizers(tmp_path):
    """pack_unit_host over the units, as sfa_pack_weights(_ex) walks them, as a stand-alone program: no ASan or UBSan
    report, every destination region written, finite, the gaps left alone (tools/pack_host_check.cpp)."""
    clang = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        pytest.skip("the ROCm clang++ is not available")
    exe = str(tmp_path / "pack_host_check")
    cmd = [clang, "-std=c++17", "-g", "-O2", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(REPO, "tools", "pack_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    sets = []
    for _, heads in pack_cases.CASES.values():  # both families run for every set
        if _set_arg(heads) not in sets:
            sets.append(_set_arg(heads))
    assert len(sets) == 3
    r = subprocess.run([exe] + sets, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and f"{len(sets)} head sets, {2 * len(sets)} packs, 0 bad" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_device_pack_is_in_the_abi():
    L = _lib.lib()
    header = open(os.path.join(REPO, "include", "sfa_hip.h")).read()
    for sym in ("sfa_pack_weights_device", "sfa_pack_weights_device_ex"):
        assert sym + "(" in header and hasattr(L, sym) and sym in _lib.EXPORTED_SYMBOLS
    assert L.sfa_abi_version() == _lib.ABI_VERSION == 2


def test_device_pack_argument_errors_need_no_device():
    """The checks that come before any device query: a null table, a wrong count, a pointer in a
    num_batches_tracked slot and a hole in the table are SFA_E_INVALID with a message."""
    L = _lib.lib()
    arch = _lib.make_arch(runtime.DEFAULT_HEADS)
    layout = _lib.state_layout(arch)
    n = len(layout)
    table = (ctypes.c_void_p * n)()
    out = ctypes.c_void_p(64)
    assert L.sfa_pack_weights_device(ctypes.byref(arch), None, n, out, None) == E_INVALID
    assert L.sfa_pack_weights_device(ctypes.byref(arch), table, n - 1, out, None) == E_INVALID
    assert b"state entries" in L.sfa_last_error_string()
    assert L.sfa_pack_weights_device(ctypes.byref(arch), table, n, out, None) == E_INVALID
    assert b"conv1.weight" in L.sfa_last_error_string()
    bad = _lib.make_arch(runtime.DEFAULT_HEADS)
    bad.num_layers = 34
    assert L.sfa_pack_weights_device(ctypes.byref(bad), table, n, out, None) == E_UNSUPPORTED
