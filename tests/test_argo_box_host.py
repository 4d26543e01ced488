"""The Argoverse box projection on the host (no GPU): the drop-in's ArgoverseCalibration gives the
reference's matrices, and the numpy restatement of the dtype chain reproduces the reference fixture
(tests/golden/gen_argo_box_golden.py) — mask and draw flag exactly, pixels within the arithmetic bound."""
import numpy as np
import pytest

import argo_box_restatement as ab
import golden_io
from conftest import GOLDEN

BOUNDARY = {"minX": -40, "maxX": 40, "minY": -40, "maxY": 40, "minZ": -3, "maxZ": 1}
D = 0.1
CALIBS = ("ident", "front")


@pytest.fixture(scope="module")
def g():
    return golden_io.load(GOLDEN, "argo_box_golden")


def fixture_calib_data(g, name):
    v = g[f"{name}/calib"]
    return ab.calib_data(v[0], v[1], v[2], v[3], v[4:7], v[7:11], v[11:14], v[14:18])


@pytest.mark.parametrize("name", CALIBS)
def test_fixture_premises(g, name):
    """What the generator asserted, checked on the committed file: no corner near the depth cut, every
    projected corner at Z_c >= 1, every category present."""
    z = g[f"{name}/cam"][..., 2]
    nan = np.isnan(g[f"{name}/pixels"][..., 0])
    assert np.all(np.abs(z - 0.1) >= 1e-3) and np.all(z[~nan] >= 1.0)
    np.testing.assert_array_equal(nan, ~(z > 0.1))
    per_box = (~nan).sum(axis=1)
    assert (per_box == 8).any() and (per_box == 0).any() and ((per_box > 0) & (per_box < 8)).any()
    np.testing.assert_array_equal(g[f"{name}/all8"], (per_box == 8).astype(np.int32))


@pytest.mark.parametrize("name", CALIBS)
def test_calibration_matches_the_reference(g, name):
    from utils.argoverse_box_utils import ArgoverseCalibration
    c = ArgoverseCalibration(fixture_calib_data(g, name))
    assert c.P2.dtype == np.float32 and c.T_l2c.dtype == np.float32
    assert c.P2.shape == (3, 4) and c.T_l2c.shape == (4, 4)
    np.testing.assert_array_equal(c.P2, g[f"{name}/P2"])
    np.testing.assert_array_equal(c.T_l2c, g[f"{name}/T_l2c"])
    assert c.camera_name == "ring_front_center" and c.camera_data["focal_length_x_px_"] == g[f"{name}/calib"][0]
    with pytest.raises(ValueError, match="Camera ring_rear_left not found in calibration."):
        ArgoverseCalibration(fixture_calib_data(g, name), "ring_rear_left")


@pytest.mark.parametrize("name", CALIBS)
def test_restatement_matches_the_fixture(g, name):
    dets, P2, T = g[f"{name}/dets"], g[f"{name}/P2"], g[f"{name}/T_l2c"]
    c3 = ab.corners(dets, BOUNDARY, D)
    assert c3.dtype == np.float32
    M = np.max(np.abs(np.concatenate([ab.metres(dets, BOUNDARY, D), dets[:, 4:7]], axis=1)), axis=1)
    assert np.all(np.abs(c3.astype(np.float64) - g[f"{name}/corners"]) <= 8 * 2.0 ** -23 * M[:, None, None])
    px = ab.project(c3.reshape(-1, 3), T, P2).reshape(-1, 8, 2)
    ref = g[f"{name}/pixels"]
    np.testing.assert_array_equal(np.isnan(px), np.isnan(ref))
    ok = ~np.isnan(ref)
    bound = ab.pixel_bound(dets, BOUNDARY, D, g[f"{name}/cam"], P2, ref)
    assert np.all(np.abs(px.astype(np.float64) - ref)[ok] <= bound[ok])
    # from the fixture's own corners the f64 chain is the same operations: the pixels within 1 ulp
    px2 = ab.project(g[f"{name}/corners"].reshape(-1, 3), T, P2).reshape(-1, 8, 2)
    assert np.all(np.abs(px2.astype(np.float64) - ref)[ok] <= ab.ulp32(ref)[ok])
