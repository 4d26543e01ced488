"""Argoverse detections -> image corners: what the reference's Argoverse scripts do between
``post_processing`` and drawing (argoverse_test2.py:260-479), without the drawing, cv2 and prints.

* ``ArgoverseCalibration(calib_data, camera_name)`` (:260-322) is host numpy, run once per log: the
  same attributes (``camera_name``, ``camera_data``, ``vehicle_SE3_lidar``, ``P2`` 3x4 float32,
  ``T_l2c`` 4x4 float32) and the same ``ValueError`` for an unknown camera.  Its
  ``project_to_image`` (:324-353) runs on the GPU (sfa_argo_project_points).
* ``create_3d_bbox_corners(dimensions, location, rotation_y)`` (:355-402) and ``box_corners`` /
  ``project_boxes`` for many detections at once run on the GPU (sfa_argo_project_boxes): float32
  corners, float64 projection, float32 pixels, NaN for a corner at camera Z <= 0.1.
* A numpy array in gives a numpy array out (one round trip through the current GPU, like
  ``makeBVFeature``); a GPU tensor in gives a GPU tensor out.  ``runtime.ArgoBoxProjector`` is the
  device-resident form that takes ``runtime.post_process``'s output for a batch.

DESIGN.md §18 has the dtype chain and the error bound against the reference's numpy arithmetic.
"""

from __future__ import annotations

import numpy as np
import torch

from sfa_hip import runtime


def _rotation_from_quaternion(q) -> np.ndarray:
    """[w, x, y, z] -> 3x3 float32 (entries computed in the coefficients' precision, then cast)."""
    w, x, y, z = q
    xx, yy, zz = x ** 2, y ** 2, z ** 2
    rows = [[1 - 2 * yy - 2 * zz, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y],
            [2 * x * y + 2 * w * z, 1 - 2 * xx - 2 * zz, 2 * y * z - 2 * w * x],
            [2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * xx - 2 * yy]]
    return np.array(rows, dtype=np.float32)


def _rigid(R, t) -> np.ndarray:
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


class ArgoverseCalibration:
    """One camera of an Argoverse 1 ``vehicle_calibration_info.json`` (already parsed)."""

    def __init__(self, calib_data, camera_name="ring_front_center"):
        self.camera_name = camera_name
        wanted = f"image_raw_{camera_name}"
        self.camera_data = next((c["value"] for c in calib_data["camera_data_"] if c["key"] == wanted), None)
        if self.camera_data is None:
            raise ValueError(f"Camera {camera_name} not found in calibration.")
        cd = self.camera_data
        self.P2 = np.array([[cd["focal_length_x_px_"], 0, cd["focal_center_x_px_"], 0],
                            [0, cd["focal_length_y_px_"], cd["focal_center_y_px_"], 0],
                            [0, 0, 1, 0]], dtype=np.float32)
        self.vehicle_SE3_lidar = calib_data["vehicle_SE3_down_lidar_"]
        self._setup_transforms()
        self._projector = None

    def _quat_to_rot_matrix(self, q):
        return _rotation_from_quaternion(q)

    def _setup_transforms(self):
        """T_l2c = (camera -> vehicle)^-1 @ (lidar -> vehicle), every matrix float32 as the scripts keep
        them; the inverse translation -R^T t is formed in float64 and stored in float32."""
        lidar = self.vehicle_SE3_lidar
        T_l2v = _rigid(_rotation_from_quaternion(np.array(lidar["rotation"]["coefficients"])),
                       np.array(lidar["translation"]))
        cam = self.camera_data["vehicle_SE3_camera_"]
        R_v2c = _rotation_from_quaternion(np.array(cam["rotation"]["coefficients"])).T
        T_v2c = _rigid(R_v2c, -R_v2c @ np.array(cam["translation"]))
        self.T_l2c = T_v2c @ T_l2v

    def projector(self, device=None, boundary=runtime.ARGO_BOUNDARY,
                  discretization: float = runtime.ARGO_DISCRETIZATION) -> "runtime.ArgoBoxProjector":
        return runtime.ArgoBoxProjector(device if device is not None else runtime.host_api_device("project_to_image"),
                                        self, boundary, discretization)

    def project_to_image(self, points_3d_lidar):
        """(n, 3) lidar-frame points -> (n, 2) float32 pixels, NaN rows where camera Z <= 0.1; an
        empty input gives the reference's empty array."""
        is_tensor = isinstance(points_3d_lidar, torch.Tensor)
        if points_3d_lidar.shape[0] == 0:
            return torch.empty(0, device=points_3d_lidar.device) if is_tensor else np.array([])
        if is_tensor:
            return self.projector(points_3d_lidar.device).project_points(points_3d_lidar)
        pts = np.ascontiguousarray(points_3d_lidar)
        if pts.dtype not in (np.float32, np.float64):
            pts = pts.astype(np.float64)  # np.hstack with float64 ones promotes integers too
        proj = self.projector()
        return proj.project_points(torch.from_numpy(pts).to(proj.device)).cpu().numpy()


def _identity_projector(device):
    class _Cam:
        T_l2c = np.eye(4, dtype=np.float32)
        P2 = np.eye(3, 4, dtype=np.float32)
    # boundary maxX = minY = minZ = 0 and d = 1 with the grid row [s, -cx, cy, cz, ...] give metres back
    zero = {"minX": 0, "maxX": 0, "minY": 0, "maxY": 0, "minZ": 0, "maxZ": 0}
    return runtime.ArgoBoxProjector(device, _Cam, zero, 1.0)


def box_corners(dims_hwl, locations, yaws):
    """create_3d_bbox_corners for n boxes: (n, 3) [h, w, l], (n, 3) [x, y, z] metres, (n,) yaw, all
    float32 -> (n, 8, 3) float32 (GPU tensors in, GPU tensor out; numpy in, numpy out)."""
    is_tensor = isinstance(dims_hwl, torch.Tensor)
    if is_tensor:
        dev = dims_hwl.device
        d, p, y = dims_hwl, locations.to(dev), yaws.to(dev)
    else:
        dev = runtime.host_api_device("create_3d_bbox_corners")
        d, p, y = (torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32))).to(dev)
                   for v in (dims_hwl, locations, yaws))
    n = int(d.shape[0])
    rows = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    # cx = 0 - x * 1 must give the location back: feed x = -location_x (exact in float32)
    rows[:, 1], rows[:, 2], rows[:, 3] = -p[:, 0].float(), p[:, 1].float(), p[:, 2].float()
    rows[:, 4:7] = d.float()
    rows[:, 7] = y.float().reshape(n)
    c3 = _identity_projector(dev)(rows, corners3d=True)[2]
    return c3 if is_tensor else c3.cpu().numpy()


def create_3d_bbox_corners(dimensions, location, rotation_y):
    """The reference's signature: (h, w, l), (x, y, z), yaw -> (8, 3) float32 corners."""
    if isinstance(dimensions, torch.Tensor):
        return box_corners(dimensions.reshape(1, 3), location.reshape(1, 3), rotation_y.reshape(1))[0]
    return box_corners(np.float32(dimensions).reshape(1, 3), np.float32(location).reshape(1, 3),
                       np.float32(rotation_y).reshape(1))[0]


def project_boxes(dets, calib, boundary=runtime.ARGO_BOUNDARY, discretization: float = runtime.ARGO_DISCRETIZATION):
    """Rows [score, x, y, z, h, w, l, yaw] (post_processing's, grid units) -> (pixels (n, 8, 2) float32,
    drawable (n,) bool): the scripts' draw_3d_bbox_on_image up to the draw call (:416-458)."""
    is_tensor = isinstance(dets, torch.Tensor)
    dev = dets.device if is_tensor else runtime.host_api_device("project_boxes")
    t = dets if is_tensor else torch.from_numpy(np.ascontiguousarray(np.asarray(dets, np.float32))).to(dev)
    px, all8, _ = runtime.ArgoBoxProjector(dev, calib, boundary, discretization)(t.reshape(-1, 8))
    ok = all8 != 0
    return (px, ok) if is_tensor else (px.cpu().numpy(), ok.cpu().numpy())
