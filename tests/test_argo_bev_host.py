"""Argoverse BEV front end (makeBVFeature, argoverse_test2.py:198-257), the checks that need no GPU:
the CPU restatement is bit-exact against every reference fixture, the C ABI's host-side entry points
(shape, scratch size, every argument error before any device call) and the drop-in's input checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import argo_bev_cases as ac
import argo_bev_restatement as ar
import golden_io
from conftest import GOLDEN, REPO
from sfa_hip import _lib

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
SCRIPT = (ctypes.c_double * 6)(-40.0, 40.0, -40.0, 40.0, -3.0, 1.0)  # argoverse_test2.py:40-47


@pytest.fixture(scope="module")
def golden_argo():
    return golden_io.load(GOLDEN, "argo_bev_golden")


@pytest.mark.parametrize("name", list(ac.cases()))
def test_restatement_bit_exact_against_reference_fixtures(golden_argo, name):
    case = ac.cases()[name]
    for k, cloud in enumerate(case["frames"]):
        ac.check_frame(golden_argo, f"{name}/{k}", ar.make_bv_feature(cloud, case["d"], case["boundary"]))


def test_cases_cover_what_they_claim(golden_argo):
    g = golden_argo
    c = ac.cases()
    assert ac.kept_fraction(c["production_800"]["frames"][0], ac.B800) >= 0.2
    assert c["production_800"]["frames"][0].shape == (100_000, 4)
    edges = ar.make_bv_feature(c["edges"]["frames"][0], 0.1, ac.B32)
    dens = edges[0]
    assert dens[26, 5] == 1.0 and dens[26, 7] == 1.0 and dens[26, 9] == np.float32(0.9)  # 10, 11 and 9 points
    assert dens[31, 10] > 0 and dens[21, 31] > 0      # x == minX -> row 31, y == maxY -> column 31 (clip)
    assert dens[11, 20] > 0 and edges[1][11, 20] == 0  # z == minZ: occupied, height 0
    assert edges[1][6, 15] == np.float32(3.75) / np.float32(4.0) and edges[2][6, 15] == np.float32(0.95) / np.float32(1.5)
    assert dens[16, 25] > 0 and edges[2][16, 25] == 0  # a negative intensity leaves 0
    zero = ar.make_bv_feature(c["zero_intensity"]["frames"][0], 0.1, ac.B32)
    assert not zero[2].any() and not np.isnan(zero).any() and zero[0].any()
    three = ar.make_bv_feature(c["three_columns"]["frames"][0], 0.1, ac.B32)
    assert np.array_equal(three[2] == 1.0, three[0] > 0)
    assert int(g["ragged4/1/nnz"]) == 0 and int(g["ragged4/2/nnz"]) == 0 and int(g["ragged4/0/nnz"]) > 0
    assert c["ragged4"]["frames"][0][:, 3].max() == 0.25 and c["ragged4"]["frames"][3][:, 3].max() == 255.0
    assert c["blocks"]["frames"][0].shape[0] >= 3000 and c["blocks"]["frames"][0].shape[0] % 1024 != 0
    n = np.round(ar.make_bv_feature(c["blocks"]["frames"][0], 0.1, ac.B64)[0] * 10)
    assert (n >= 10).sum() >= 50  # many cells at the density cap


def _shape(bnd, d):
    H, W = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.lib().sfa_argo_bev_shape(bnd, d, ctypes.byref(H), ctypes.byref(W))
    return rc, H.value, W.value


def test_shape_follows_python_double_arithmetic():
    assert _shape(SCRIPT, 0.1) == (0, 800, 800)
    for case in ac.cases().values():
        b = case["boundary"]
        arr = (ctypes.c_double * 6)(*[b[k] for k in ("minX", "maxX", "minY", "maxY", "minZ", "maxZ")])
        assert _shape(arr, case["d"]) == (0,) + tuple(case["shape"])
    assert ac.cases()["ragged4"]["shape"] == (64, 48)
    # int(4.8 / 0.1) is 47 in Python (47.99999999999999): the C side must truncate the same double
    assert int(4.8 / 0.1) == 47
    assert _shape((ctypes.c_double * 6)(0.0, 6.4, 0.0, 4.8, -3.0, 1.0), 0.1) == (0, 64, 47)
    from sfa_hip import runtime
    assert runtime.argo_bev_shape(ac.BPIPE, 0.1) == (160, 128)
    assert runtime.argo_bev_shape(runtime.ARGO_BOUNDARY, runtime.ARGO_DISCRETIZATION) == (800, 800)


def test_symbols_exported_bound_and_declared():
    L = _lib.lib()
    hdr = open(os.path.join(REPO, "include", "sfa_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in ("sfa_argo_bev_shape", "sfa_argo_bev_scratch_size", "sfa_argo_bev_voxelize"):
        assert hasattr(L, s), s
        assert s in _lib.EXPORTED_SYMBOLS and getattr(L, s).argtypes is not None
        assert re.search(r"\b" + s + r"\s*\(", code), f"{s} not declared in include/sfa_hip.h"
    assert re.search(r"#define\s+SFA_ABI_VERSION\s+2\b", hdr) and L.sfa_abi_version() == 2
    assert f"#define SFA_ARGO_BEV_MAX_DIM {_lib.ARGO_BEV_MAX_DIM}" in hdr
    assert f"#define SFA_ARGO_BEV_FORCE_ATOMIC 0x{_lib.ARGO_BEV_FORCE_ATOMIC:x}" in hdr


def test_scratch_size():
    L = _lib.lib()
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for b, h, w in ((1, 800, 800), (16, 800, 800), (4, 64, 48), (1, 608, 608), (64, 2048, 2048), (1, 1, 1)):
        assert L.sfa_argo_bev_scratch_size(b, h, w) == 2 * (256 + al(b * h * w * 12)), (b, h, w)
    for b, h, w in ((0, 800, 800), (65, 800, 800), (1, 0, 800), (1, 800, 2049), (-1, 8, 8)):
        assert L.sfa_argo_bev_scratch_size(b, h, w) == 0, (b, h, w)


def test_argument_errors_before_any_device_call():
    """Every bad argument returns its documented status with the reason set; the buffers are host
    memory, so a launch would fault — none happens."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    offs = (ctypes.c_int64 * 2)(0, 10)
    B32 = (ctypes.c_double * 6)(0.0, 3.2, 0.0, 3.2, -3.0, 1.0)
    big = L.sfa_argo_bev_scratch_size(1, 32, 32)

    def vox(points=p, stride=4, offsets=offs, batch=1, bnd=B32, d=0.1, layout=_lib.BEV_NCHW3_F32, out=p,
            scratch=p, nbytes=big):
        return L.sfa_argo_bev_voxelize(points, stride, offsets, batch, bnd, d, layout, out, scratch, nbytes, None)

    def err():
        return L.sfa_last_error_string()

    assert vox(batch=0) == INVALID and b"batch" in err()
    assert vox(batch=65) == INVALID and b"batch" in err()
    assert vox(offsets=None) == INVALID and b"null" in err()
    assert vox(bnd=None) == INVALID and b"null" in err()
    assert vox(out=None) == INVALID and b"null" in err()
    assert vox(scratch=None) == INVALID and b"null" in err()
    assert vox(points=None) == INVALID and b"null points" in err()
    for stride in (2, 1, 0, -4):
        assert vox(stride=stride) == INVALID and b"point_stride" in err(), stride
    for d in (0.0, -0.1, float("nan"), float("inf")):
        assert vox(d=d) == INVALID and b"discretization" in err(), d
    for bad in ((3.2, 0.0, 0.0, 3.2, -3.0, 1.0), (0.0, 3.2, 3.2, 3.2, -3.0, 1.0), (0.0, 3.2, 0.0, 3.2, 1.0, -3.0)):
        assert vox(bnd=(ctypes.c_double * 6)(*bad)) == INVALID and b"inverted" in err(), bad
    assert vox(bnd=(ctypes.c_double * 6)(0.0, float("nan"), 0.0, 3.2, -3.0, 1.0)) == INVALID
    assert vox(layout=_lib.BEV_NCHW3_F64) == INVALID and b"out_layout" in err()
    assert vox(layout=7) == INVALID and b"out_layout" in err()
    assert vox(offsets=(ctypes.c_int64 * 2)(10, 0)) == INVALID and b"monotone" in err()
    assert vox(offsets=(ctypes.c_int64 * 2)(-1, 5)) == INVALID
    assert vox(offsets=(ctypes.c_int64 * 2)(0, 1 << 32)) == UNSUPPORTED and b"points" in err()
    assert vox(nbytes=big - 1) == WORKSPACE and b"scratch" in err()
    assert vox(nbytes=0) == WORKSPACE
    assert vox(batch=2, offsets=(ctypes.c_int64 * 3)(0, 5, 10)) == WORKSPACE  # sized for one frame
    # maps the kernels do not cover: more than 2048 cells a side, or none
    assert vox(d=0.001) == UNSUPPORTED and b"2048" in err()
    assert vox(d=5.0) == UNSUPPORTED
    assert vox(scratch=ctypes.c_void_p(p.value + 4)) == INVALID and b"aligned" in err()
    # the shape entry point reports the same
    H, W = ctypes.c_int(), ctypes.c_int()
    assert L.sfa_argo_bev_shape(None, 0.1, ctypes.byref(H), ctypes.byref(W)) == INVALID
    assert L.sfa_argo_bev_shape(B32, 0.1, None, ctypes.byref(W)) == INVALID
    assert L.sfa_argo_bev_shape(B32, 0.0, ctypes.byref(H), ctypes.byref(W)) == INVALID
    assert L.sfa_argo_bev_shape(B32, 0.001, ctypes.byref(H), ctypes.byref(W)) == UNSUPPORTED
    assert L.sfa_argo_bev_shape((ctypes.c_double * 6)(-102.4, 102.4, -102.4, 102.4, -3.0, 1.0), 0.1,
                                ctypes.byref(H), ctypes.byref(W)) == 0 and (H.value, W.value) == (2048, 2048)


def test_dropin_input_checks_need_no_device():
    from data_process.argoverse_bev_utils import makeBVFeature
    with pytest.raises(ValueError, match="Invalid point cloud shape"):
        makeBVFeature(np.zeros((5, 2), np.float32), 0.1, ac.B32)
    with pytest.raises(ValueError):
        makeBVFeature(np.zeros(8, np.float32), 0.1, ac.B32)
    with pytest.raises(TypeError, match="float32"):
        makeBVFeature(np.zeros((5, 4), np.float64), 0.1, ac.B32)
    import torch
    with pytest.raises(TypeError, match="float32"):
        makeBVFeature(torch.zeros((5, 4), dtype=torch.float64), 0.1, ac.B32)
    with pytest.raises(_lib.SfaNativeError):  # a CPU tensor: there is no CPU fallback
        makeBVFeature(torch.zeros((5, 4)), 0.1, ac.B32)


def test_pipeline_option_checks():
    from sfa_hip import runtime
    with pytest.raises(ValueError, match="bev must be"):
        runtime.DetectorPipeline(None, 1, bev="nuscenes")
    with pytest.raises(ValueError, match="with_bev"):
        runtime.DetectorPipeline(None, 1, bev="argoverse")
    with pytest.raises(ValueError, match="discretization"):
        runtime.DetectorPipeline(None, 1, discretization=0.1)
