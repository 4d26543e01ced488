"""sfa_argo_project_boxes / sfa_argo_project_points against the reference fixture
(tests/golden/gen_argo_box_golden.py): the NaN mask and the all-eight flag exactly, the pixels within the
per-corner bound of argo_box_restatement.pixel_bound, which is derived from the arithmetic (three float32
steps of at most about 2 ulp of the coordinate magnitude each, carried through the projection's
derivative), not fitted to the kernel.  Largest observed error / bound on an MI355X: see DESIGN.md §18.
"""
import numpy as np
import pytest
import torch

import argo_box_restatement as ab
import golden_io
from conftest import GOLDEN
from sfa_hip import runtime
from test_argo_box_host import BOUNDARY, CALIBS, D, fixture_calib_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return golden_io.load(GOLDEN, "argo_box_golden")


def _calib(g, name):
    from utils.argoverse_box_utils import ArgoverseCalibration
    return ArgoverseCalibration(fixture_calib_data(g, name))


@pytest.mark.parametrize("name", CALIBS)
def test_boxes_match_the_reference(g, gpu, name):
    dets, ref = g[f"{name}/dets"], g[f"{name}/pixels"]
    proj = runtime.ArgoBoxProjector(gpu, _calib(g, name), BOUNDARY, D)
    px, all8, c3 = proj(torch.from_numpy(dets).to(gpu), corners3d=True)
    px, all8, c3 = px.cpu().numpy(), all8.cpu().numpy(), c3.cpu().numpy()
    assert px.dtype == np.float32 and px.shape == ref.shape and all8.dtype == np.int32
    np.testing.assert_array_equal(np.isnan(px), np.isnan(ref))
    np.testing.assert_array_equal(all8, g[f"{name}/all8"])
    ok = ~np.isnan(ref)
    err = np.abs(px.astype(np.float64) - ref)
    bound = ab.pixel_bound(dets, BOUNDARY, D, g[f"{name}/cam"], g[f"{name}/P2"], ref)
    ratio = float(np.max(err[ok] / bound[ok]))
    print(f"argo_project_boxes[{name}]: max |err| {err[ok].max():.3e} px, max err / bound {ratio:.3f}")
    assert ratio <= 1.0
    M = np.max(np.abs(np.concatenate([ab.metres(dets, BOUNDARY, D), dets[:, 4:7]], axis=1)), axis=1)
    assert np.all(np.abs(c3.astype(np.float64) - g[f"{name}/corners"]) <= 8 * 2.0 ** -23 * M[:, None, None])


def test_offsets_limit_the_rows(g, gpu):
    """With post_process' device offsets only rows [0, offsets[B]) are written."""
    dets = torch.from_numpy(g["front/dets"]).to(gpu)
    n = dets.shape[0]
    proj = runtime.ArgoBoxProjector(gpu, _calib(g, "front"), BOUNDARY, D)
    full = proj(dets)
    out = (torch.full((n, 8, 2), 7.0, device=gpu), torch.full((n,), 7, dtype=torch.int32, device=gpu), None)
    offs = torch.tensor([0, 5, 13], dtype=torch.int32, device=gpu)
    px, all8, _ = proj(dets, offs, out=out)
    np.testing.assert_array_equal(px[:13].cpu().numpy().view(np.uint32), full[0][:13].cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(all8[:13].cpu().numpy(), full[1][:13].cpu().numpy())
    assert bool((px[13:] == 7.0).all()) and bool((all8[13:] == 7).all())


def test_pipeline_rows_project(gpu):
    """The device output of post_process goes straight in (no host hop)."""
    rng = np.random.default_rng(2)
    d = rng.random((2, 20, 10), dtype=np.float32)
    d[..., 9] = rng.integers(0, 3, (2, 20))
    d[..., 1:3] *= 200
    d[..., 3] *= 20  # depths on both sides of the cut (identity calibration: camera Z = lidar z)
    preds, _, off = runtime.post_process(torch.from_numpy(d).to(gpu), peak_thresh=0.5)
    cal = type("C", (), {"T_l2c": np.eye(4, dtype=np.float32), "P2": np.eye(3, 4, dtype=np.float32)})
    px, all8, _ = runtime.ArgoBoxProjector(gpu, cal, BOUNDARY, D)(preds, off)
    n = int(off[-1])
    exp = ab.project(ab.corners(preds[:n].cpu().numpy(), BOUNDARY, D).reshape(-1, 3), cal.T_l2c, cal.P2).reshape(n, 8, 2)
    np.testing.assert_array_equal(np.isnan(px[:n].cpu().numpy()), np.isnan(exp))
    np.testing.assert_array_equal(all8[:n].cpu().numpy(), (~np.isnan(exp).any(axis=(1, 2))).astype(np.int32))


@pytest.mark.parametrize("name", CALIBS)
def test_dropin_functions(g, gpu, name):
    """utils.argoverse_box_utils: numpy in, numpy out (one round trip); GPU tensor in, GPU tensor out."""
    from utils import argoverse_box_utils as u
    calib = _calib(g, name)
    dets, c3 = g[f"{name}/dets"], g[f"{name}/corners"]
    ref = g[f"{name}/pixels"]
    pts = c3.reshape(-1, 3)
    px = calib.project_to_image(pts)
    assert isinstance(px, np.ndarray) and px.dtype == np.float32 and px.shape == (pts.shape[0], 2)
    np.testing.assert_array_equal(np.isnan(px), np.isnan(ref.reshape(-1, 2)))
    ok = ~np.isnan(ref.reshape(-1, 2))
    assert np.all(np.abs(px.astype(np.float64) - ref.reshape(-1, 2))[ok] <= ab.ulp32(ref.reshape(-1, 2))[ok])
    px64 = calib.project_to_image(pts.astype(np.float64))
    np.testing.assert_array_equal(px64.view(np.uint32), px.view(np.uint32))
    t = calib.project_to_image(torch.from_numpy(pts).to(gpu))
    assert t.device == gpu
    np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), px.view(np.uint32))
    assert calib.project_to_image(np.zeros((0, 3), np.float32)).size == 0
    m = ab.metres(dets, BOUNDARY, D)
    one = u.create_3d_bbox_corners(tuple(dets[0, 4:7]), tuple(m[0]), dets[0, 7])
    assert one.shape == (8, 3) and one.dtype == np.float32
    M = float(np.max(np.abs(np.concatenate([m[0], dets[0, 4:7]]))))
    assert np.all(np.abs(one.astype(np.float64) - c3[0]) <= 8 * 2.0 ** -23 * M)
    pxb, drawable = u.project_boxes(dets, calib, BOUNDARY, D)
    np.testing.assert_array_equal(drawable, g[f"{name}/all8"] != 0)
    np.testing.assert_array_equal(np.isnan(pxb), np.isnan(ref))
