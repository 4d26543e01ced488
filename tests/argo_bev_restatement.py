"""Independent CPU restatement of the reference's makeBVFeature (argoverse_test2.py:198-257) in
vectorised numpy: the Python loop's two running maxima and its counter become np.maximum.at and
np.bincount.  Bit-exact against every fixture (tests/test_argo_bev_host.py); the GPU tests use it
for the cases that have no fixture.  float32 points only, like the GPU path."""
import numpy as np

F = np.float32


def make_bv_feature(points, discretization, boundary):
    """(N, 3) or (N, >= 4) float32 -> (3, H, W) float32, channels (density, height, intensity)."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] < 3:
        raise ValueError(f"Invalid point cloud shape: {points.shape}")
    if points.dtype != F:
        raise TypeError("float32 points only")
    H = int((boundary["maxX"] - boundary["minX"]) / discretization)
    W = int((boundary["maxY"] - boundary["minY"]) / discretization)
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    i = points[:, 3] if points.shape[1] >= 4 else np.full(x.shape, 0.5, F)
    lo = [F(boundary[k]) for k in ("minX", "minY", "minZ")]
    hi = [F(boundary[k]) for k in ("maxX", "maxY", "maxZ")]
    keep = (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
    x, y, z, i = x[keep], y[keep], z[keep], i[keep]
    d = F(discretization)
    row = np.clip(((hi[0] - x) / d).astype(np.int32), 0, H - 1)
    col = np.clip(((y - lo[1]) / d).astype(np.int32), 0, W - 1)
    cell = row.astype(np.int64) * W + col
    h = np.zeros(H * W, F)
    np.maximum.at(h, cell, z - lo[2])                    # z - minZ >= +0 after the box test
    im = np.zeros(H * W, F)
    np.maximum.at(im, cell, np.where(i > 0, i, F(0)))   # Python's max(0, i): NaN and negatives never win
    n = np.bincount(cell, minlength=H * W)
    dens = np.minimum(n.astype(F) / F(10.0), F(1.0))
    if h.size and h.max() > 0:
        h = h / F(boundary["maxZ"] - boundary["minZ"])   # the difference in double, as Python takes it
    if im.size and im.max() > 0:
        im = im / im.max()
    return np.stack([dens, h, im]).reshape(3, H, W).astype(F)
