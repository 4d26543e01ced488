"""Drop-in for the ``makeBVFeature`` the reference's Argoverse scripts define themselves
(argoverse_test2.py:198-257; argoverse_test.py:199-254 and argo_sfa_test.py carry the same function).

``makeBVFeature(points, discretization, boundary)`` keeps the reference's signature and result —
a (3, H, W) float32 map, channels [density, height, intensity], H = int((maxX - minX) / d),
W = int((maxY - minY) / d) — but the voxelisation runs on the GPU (sfa_argo_bev_voxelize,
bit-exact against the Python loop).  A numpy array in gives a numpy array out; a GPU
tensor in gives a GPU tensor out (no host hop).

Points must be float32: the kernels reproduce numpy's float32 arithmetic, and a float64 cloud goes
through float64 arithmetic in the reference, which they do not restate — such input raises
``TypeError`` (convert with ``points.astype(np.float32)``, which is what a PLY / .bin sweep holds
anyway).  Fewer than 3 columns raise ``ValueError`` like the reference (:207).
"""

from __future__ import annotations

import numpy as np
import torch

from sfa_hip import _lib, runtime


def makeBVFeature(points, discretization, boundary, device=None):
    """(N, 3) or (N, >= 4) float32 points -> (3, H, W) float32 BEV map (GPU tensor for a GPU tensor,
    numpy for numpy).  With 3 columns every point has intensity 0.5 (:201-203)."""
    is_tensor = isinstance(points, torch.Tensor)
    if not is_tensor:
        points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] < 3:
        raise ValueError(f"Invalid point cloud shape: {tuple(points.shape)}")
    if points.dtype != (torch.float32 if is_tensor else np.float32):
        raise TypeError(f"makeBVFeature: points must be float32, got {points.dtype}")
    if is_tensor:
        t = runtime._require_gpu_tensor(points, "makeBVFeature")  # a CPU tensor is refused: no CPU fallback
    else:
        dev = runtime.host_api_device("makeBVFeature", device)
        t = torch.from_numpy(np.ascontiguousarray(points)).to(dev)
    out = runtime.argo_voxelizer(t.device, boundary, discretization)(t, [0, t.shape[0]],
                                                                     layout=_lib.BEV_NCHW3_F32)[0]
    return out if is_tensor else out.cpu().numpy()


def makeBVFeatureBatch(points: torch.Tensor, offsets, discretization, boundary, layout: str = "nchw3"):
    """B sweeps packed back to back (offsets: B + 1 ints) on the device -> (B, 3, H, W) or, with
    layout "nhwc4", the model's (B, H, W, 4) input (channel 3 = 0)."""
    lay = _lib.BEV_NHWC4_F32 if layout == "nhwc4" else _lib.BEV_NCHW3_F32
    return runtime.argo_voxelizer(points.device, boundary, discretization)(points, offsets, layout=lay)
