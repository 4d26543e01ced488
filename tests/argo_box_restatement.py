"""CPU restatement of the Argoverse scripts' box projection (argoverse_test2.py:260-479 without
drawing) — TEST INFRASTRUCTURE ONLY — and the error bound of tests/test_gpu_argo_box.py.

Dtype chain, as numpy >= 2 runs the reference: grid -> metres and the eight corners in float32
(f32 cos / sin, a 3x3 @ 3x8 float32 product, one float32 add of the location); hstack with float64
ones promotes, so the 4x4 and 3x4 transforms and the divide are float64; the result array is float32.
"""
import numpy as np

CORNER_SIGNS = np.array([[1, 1, -1, -1, 1, 1, -1, -1],      # +-l/2 along the box's first axis
                         [0, 0, 0, 0, -1, -1, -1, -1],      # 0 or -h along the second
                         [1, -1, -1, 1, 1, -1, -1, 1]])     # +-w/2 along the third


def calib_data(fx, fy, cx, cy, lidar_t, lidar_q, cam_t, cam_q, camera="ring_front_center"):
    """The slice of an Argoverse 1 vehicle_calibration_info.json that the scripts read."""
    se3 = lambda t, q: {"translation": [float(v) for v in t], "rotation": {"coefficients": [float(v) for v in q]}}
    return {"camera_data_": [{"key": f"image_raw_{camera}",
                              "value": {"focal_length_x_px_": float(fx), "focal_length_y_px_": float(fy),
                                        "focal_center_x_px_": float(cx), "focal_center_y_px_": float(cy),
                                        "vehicle_SE3_camera_": se3(cam_t, cam_q)}}],
            "vehicle_SE3_down_lidar_": se3(lidar_t, lidar_q)}


def metres(dets, boundary, d):
    """(n, 8) f32 rows [score, x, y, z, h, w, l, yaw] -> (n, 3) f32 [cx, cy, cz]."""
    dets = np.asarray(dets, np.float32)
    f = np.float32
    return np.stack([f(boundary["maxX"]) - dets[:, 1] * f(d), dets[:, 2] * f(d) + f(boundary["minY"]),
                     dets[:, 3] + f(boundary["minZ"])], axis=1).astype(np.float32)


def corners(dets, boundary, d):
    """(n, 8, 3) f32 box corners in the lidar frame."""
    dets = np.asarray(dets, np.float32)
    loc = metres(dets, boundary, d)
    half = np.stack([dets[:, 6] / 2, dets[:, 4], dets[:, 5] / 2], axis=1).astype(np.float32)  # l/2, h, w/2
    local = CORNER_SIGNS[None].astype(np.float32) * half[:, :, None]                          # (n, 3, 8)
    c, s = np.cos(dets[:, 7]), np.sin(dets[:, 7])                                             # f32
    X = (c[:, None] * local[:, 0] + s[:, None] * local[:, 2]) + loc[:, 0:1]
    Y = local[:, 1] + loc[:, 1:2]
    Z = (-s[:, None] * local[:, 0] + c[:, None] * local[:, 2]) + loc[:, 2:3]
    return np.stack([X, Y, Z], axis=2).astype(np.float32)


def camera_frame(points, T_l2c):
    """(m, 3) -> (m, 4) f64 rows T_l2c @ [x, y, z, 1]."""
    hom = np.concatenate([np.asarray(points, np.float64), np.ones((len(points), 1))], axis=1)
    return hom @ np.asarray(T_l2c, np.float64).T


def project(points, T_l2c, P2):
    """(m, 3) -> (m, 2) f32 pixels, NaN rows where the camera depth is <= 0.1."""
    cam = camera_frame(points, T_l2c)
    pr = cam @ np.asarray(P2, np.float64).T
    out = np.full((len(points), 2), np.nan, np.float32)
    ok = cam[:, 2] > 0.1
    out[ok] = (pr[ok, :2] / pr[ok, 2:3]).astype(np.float32)
    return out


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def pixel_bound(dets, boundary, d, cam, P2, pixels):
    """Per-corner bound on |pixel - fixture pixel| for an implementation that follows the dtype chain
    with its own f32 cos / sin, product order and FMA choices: each of the three f32 steps (cos / sin,
    the 3x3 @ 3x8 product, the add of the location) moves a lidar coordinate by at most about 2 ulp of
    the coordinate magnitude M = max(|cx|, |cy|, |cz|, l, w, h) — 8 * 2^-23 * M with margin for their
    combination — and a lidar-frame displacement e moves a pixel by at most (f / Z)(1 + |X| / Z) e
    (the derivative of f X / Z in X and in Z; T_l2c is a rigid motion).  2 ulp of the pixel for the
    final rounding.  cam: (n, 8, 4) f64 from the fixture; returns (n, 8, 2)."""
    dets = np.asarray(dets, np.float32)
    M = np.max(np.abs(np.concatenate([metres(dets, boundary, d), dets[:, 4:7]], axis=1)).astype(np.float64), axis=1)
    Z = cam[..., 2]
    e = 8 * 2.0 ** -23 * M[:, None]
    P2 = np.asarray(P2, np.float64)
    bu = P2[0, 0] / Z * (1 + np.abs(cam[..., 0]) / Z) * e + 2 * ulp32(pixels[..., 0])
    bv = P2[1, 1] / Z * (1 + np.abs(cam[..., 1]) / Z) * e + 2 * ulp32(pixels[..., 1])
    return np.stack([bu, bv], axis=-1)
