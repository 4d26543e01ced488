"""Inputs of the Argoverse BEV (makeBVFeature, argoverse_test2.py:198-257) fixtures and tests: each
case is the smallest map at which its path can still go wrong.  Shared by
tests/golden/gen_argo_bev_golden.py (which runs the reference on them), the CPU restatement test and
the GPU tests; everything is regenerated from seeds (sfa_hip.synthetic) or written out by hand."""
import hashlib

import numpy as np

from sfa_hip import synthetic

F = np.float32


def _bnd(x0, x1, y0, y1, z0=-3.0, z1=1.0):
    return {"minX": x0, "maxX": x1, "minY": y0, "maxY": y1, "minZ": z0, "maxZ": z1}


B32 = _bnd(0.0, 3.2, 0.0, 3.2)          # 32 x 32 at d = 0.1
B64x48 = _bnd(0.0, 6.4, 0.0, 4.85)      # 64 x 48: H != W (4.8 / 0.1 is 47.99999999999999 in double: W = 47)
B64 = _bnd(0.0, 6.4, 0.0, 6.4)          # 64 x 64
B015 = _bnd(-4.8, 4.8, -4.8, 4.8)       # d = 0.15: every division rounds
B800 = _bnd(-40.0, 40.0, -40.0, 40.0)   # the scripts' config: 800 x 800 at d = 0.1
BKITTI = _bnd(0.0, 50.0, -25.0, 25.0, -2.73, 1.27)
D_KITTI = 0.0822                        # 50 / 0.0822 = 608.27 -> 608 x 608
BPIPE = _bnd(0.0, 16.0, 0.0, 12.8)      # 160 x 128: the pipeline test's map (multiples of 32)


def _uniform(seed, stream, n, lo, hi):
    return (lo + (hi - lo) * synthetic.hash_uniform(seed, stream, n)).astype(F)


def random_cloud(seed, n, bnd, margin=0.3, i_lo=0.0, i_hi=1.0, cols=4):
    """n points uniform over the box grown by ``margin`` metres on every side (so some are dropped)."""
    c = np.empty((n, cols), F)
    c[:, 0] = _uniform(seed, 1, n, bnd["minX"] - margin, bnd["maxX"] + margin)
    c[:, 1] = _uniform(seed, 2, n, bnd["minY"] - margin, bnd["maxY"] + margin)
    c[:, 2] = _uniform(seed, 3, n, bnd["minZ"] - margin, bnd["maxZ"] + margin)
    if cols >= 4:
        c[:, 3] = _uniform(seed, 4, n, i_lo, i_hi)
    for k in range(4, cols):
        c[:, k] = _uniform(seed, 1 + k, n, -5.0, 5.0)  # extra columns are ignored
    return c


def edges_cloud():
    """Hand-written 32 x 32 case: the closed bounds, the clip, density 10 / 11, independent maxima."""
    up = lambda v: np.nextafter(F(v), F(np.inf))    # noqa: E731
    dn = lambda v: np.nextafter(F(v), F(-np.inf))   # noqa: E731
    p = []
    # exactly on the six closed bounds: x == minX -> row 31 through the clip ((3.2 - 0) / 0.1 = 32),
    # x == maxX -> row 0, y == maxY -> column 31 through the clip, y == minY -> column 0
    p += [(0.0, 1.05, -1.0, 0.5), (3.2, 1.05, -1.0, 0.6), (1.05, 3.2, -1.0, 0.7), (1.05, 0.0, -1.0, 0.8)]
    p += [(2.05, 2.05, -3.0, 0.9)]   # z == minZ: height exactly 0 in an occupied cell
    p += [(2.05, 2.25, 1.0, 0.3)]    # z == maxZ: height exactly 1
    p += [(0.0, 0.0, -3.0, 0.0), (3.2, 3.2, 1.0, 1.5)]  # corners of the box
    # just outside each bound: dropped
    p += [(dn(0.0), 1.0, 0.0, 9.0), (up(3.2), 1.0, 0.0, 9.0), (1.0, dn(0.0), 0.0, 9.0), (1.0, up(3.2), 0.0, 9.0),
          (1.0, 1.0, dn(-3.0), 9.0), (1.0, 1.0, up(1.0), 9.0), (np.nan, 1.0, 0.0, 9.0), (1.0, 1.0, np.nan, 9.0)]
    # a cell with exactly 10 points (density exactly 1.0) and one with 11 (clipped to 1.0), 9 -> 0.9
    p += [(0.55, 0.55, -2.0 + 0.1 * k, 0.01 * k) for k in range(10)]
    p += [(0.55, 0.75, -2.0 + 0.1 * k, 0.01 * k) for k in range(11)]
    p += [(0.55, 0.95, -2.0 + 0.1 * k, 0.01 * k) for k in range(9)]
    p += [(2.55, 0.55, 0.25, 0.4)]   # a cell with 1 point
    # the max-z point is not the max-intensity point
    p += [(2.55, 1.55, 0.75, 0.1), (2.56, 1.56, -2.5, 0.95), (2.57, 1.57, 0.0, 0.2)]
    # negative, -0 and NaN intensities never beat the initial 0
    p += [(1.55, 2.55, 0.0, -7.0), (1.55, 2.75, 0.0, -0.0), (1.55, 2.95, 0.0, np.nan),
          (1.55, 3.05, 0.0, -3.0), (1.56, 3.05, -1.0, 0.125)]
    # on interior cell borders (the division decides the cell)
    p += [(1.0, 2.0, -0.5, 0.33), (0.3, 0.7, -0.5, 0.44), (2.9, 1.1, -0.5, 0.55)]
    return np.array(p, dtype=F)


def dense_cloud(seed, n, bnd):
    """Half the points in a 1.2 m x 1.2 m cluster (cells with n > 10), half spread over the box."""
    c = random_cloud(seed, n, bnd, i_hi=2.0)
    k = n // 2
    c[:k, 0] = _uniform(seed, 11, k, 2.0, 3.2)
    c[:k, 1] = _uniform(seed, 12, k, 3.0, 4.2)
    return c


def production_sweep(seed=1, n=100_000):
    """synthetic's KITTI-like sweep (rings to 80 m) rescaled into the Argoverse box: x, y halved,
    intensity 0..255 as Argoverse stores it, n points taken evenly."""
    return synthetic.synthetic_argoverse_sweep(seed, n)


def kept_fraction(c, bnd):
    m = ((c[:, 0] >= F(bnd["minX"])) & (c[:, 0] <= F(bnd["maxX"])) & (c[:, 1] >= F(bnd["minY"])) &
         (c[:, 1] <= F(bnd["maxY"])) & (c[:, 2] >= F(bnd["minZ"])) & (c[:, 2] <= F(bnd["maxZ"])))
    return float(m.mean()) if m.size else 0.0


def cases():
    """{name: {"frames": [clouds], "boundary": dict, "d": float, "shape": (H, W)}} in the issue's order."""
    out = {}
    out["edges"] = dict(frames=[edges_cloud()], boundary=B32, d=0.1, shape=(32, 32))
    zero = random_cloud(21, 300, B32)
    zero[:, 3] = 0.0
    out["zero_intensity"] = dict(frames=[zero], boundary=B32, d=0.1, shape=(32, 32))
    out["three_columns"] = dict(frames=[random_cloud(22, 300, B32, cols=3)], boundary=B32, d=0.1, shape=(32, 32))
    typical = random_cloud(23, 900, B64x48, i_hi=0.25)
    typical[7, 3] = 0.25
    outside = random_cloud(24, 200, B64x48)
    outside[:, 2] += F(10.0)                       # empty after the filter
    bright = random_cloud(25, 700, B64x48, i_lo=-1.0, i_hi=200.0, cols=5)
    bright[11, :3] = (3.0, 2.0, 0.0)
    bright[11, 3] = 255.0
    out["ragged4"] = dict(frames=[typical, outside, np.zeros((0, 4), F), bright[:, :4].copy()], boundary=B64x48,
                          d=0.1, shape=(64, 48))
    out["blocks"] = dict(frames=[dense_cloud(26, 3500, B64), dense_cloud(27, 1700, B64)], boundary=B64, d=0.1,
                         shape=(64, 64))
    out["inexact_d"] = dict(frames=[random_cloud(28, 2000, B015, i_lo=-1.0, i_hi=3.0)], boundary=B015, d=0.15,
                            shape=(64, 64))
    out["production_800"] = dict(frames=[production_sweep()], boundary=B800, d=0.1, shape=(800, 800))
    out["kitti_608"] = dict(frames=[synthetic.synthetic_point_cloud(2)], boundary=BKITTI, d=D_KITTI,
                            shape=(608, 608))
    return out


SHA_ONLY = ("production_800", "kitti_608")  # stored as SHA-256 + a COO sample (the file stays < 1 MiB)


def random_clouds(count=20, seed0=100):
    """Seeded 64 x 64 clouds of 0 - 5,000 points, intensities in [-1, 300), for the restatement-vs-GPU test."""
    out = []
    for k in range(count):
        n = int(synthetic.hash_uniform(seed0 + k, 9, 1)[0] * 5001) if k else 0
        out.append(random_cloud(seed0 + k, n, B64, i_lo=-1.0, i_hi=300.0))
    return out


def check_frame(g, key, got):
    """``got`` (3, H, W) f32 equals the fixture frame ``key`` = "<case>/<frame>" bit for bit."""
    case = key.split("/")[0]
    assert got.dtype == np.float32 and got.shape == (3,) + tuple(int(v) for v in g[f"{key}/hw"]), key
    flat = np.ascontiguousarray(got).reshape(-1)
    if case not in SHA_ONLY:  # the whole map from its COO form, compared as bits
        exp = np.zeros(flat.size, np.float32)
        exp[g[f"{key}/idx"]] = g[f"{key}/val"]
        np.testing.assert_array_equal(flat.view(np.uint32), exp.view(np.uint32), err_msg=key)
    else:
        np.testing.assert_array_equal(flat[g[f"{key}/idx"]].view(np.uint32), g[f"{key}/val"].view(np.uint32),
                                      err_msg=key)
        assert int(np.count_nonzero(flat.view(np.uint32))) == int(g[f"{key}/nnz"]), key
    assert hashlib.sha256(flat.tobytes()).hexdigest() == str(g[f"{key}/sha"]), key
