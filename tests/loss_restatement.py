"""numpy restatement, with every dtype explicit, of the reference's validation tier:
``build_targets`` (data_process/kitti_dataset.py:157-244 with compute_radius, gaussian2D and gen_hm_radius,
kitti_data_utils.py:176-225) and ``compute_loss`` (losses/losses.py:44-163, in float64).

Dtypes of build_targets, stated once.  The reference unpacks a float32 label row into numpy float32
scalars and combines them with Python numbers.  Under numpy >= 2 (NEP 50; the fixtures were generated with
the numpy version recorded in them) a float32 scalar (op) a Python int or float STAYS float32, and a
comparison converts the Python number to float32.  So, with F = np.float32:
  * the boundary test compares x, y, z with F(minX) ... F(maxZ) (z == F(-2.73) is inside, although
    F(-2.73) < -2.73 in float64);
  * bbox_l = l / F(bound_size_x) * F(hm_l) and bbox_w likewise, in float32; math.ceil gives Python ints;
  * compute_radius runs on Python ints and floats, i.e. in float64 (np.sqrt of a Python float is float64);
    radius = max(0, int(.)) truncates;
  * center_y = (x - F(minX)) / F(bound_size_x) * F(hm_l), center_x likewise, float32; the h-flip is
    F(hm_w) - center_x - F(1) in float32; center_int truncates toward zero;
  * the gaussian is float64: exp(-(dx*dx + dy*dy) / (2 * sigma * sigma)), sigma = (2r + 1) / 6, nothing is
    below eps * max for these sigmas; np.maximum(float32 map, float64 gaussian, out=float32 map) is
    max(map, F(gaussian)) since rounding is monotone;
  * center - center_int is float32 - int32 = float64, exact, stored as float32 (the same value as the
    float32 difference);
  * direction = F(math.sin(float(yaw))), F(math.cos(float(yaw))) with yaw = -label yaw in float32;
  * z_coor = z - F(minZ) in float32; dim = h, w, l.
The slices of gen_hm_radius clip the gaussian to the map for a centre on or one cell past an edge
(center_int[1] == hm_l when x == maxX; center_int[0] == -1 when a flipped y == maxY): the clipped patch is
`|dx| <= r and |dy| <= r` intersected with the map, which is how it is restated.  Where the reference
cannot go on (a class id outside [-num_classes - 1, num_classes): IndexError; the 0.9999 assignment of an
ignore label whose centre is outside the map: IndexError, or a wrap to the last column for -1) the
restatement, like the kernel, skips that write and reports it in ``status`` (bit 1 / bit 0).
"""
import math

import numpy as np

F = np.float32
KEYS = ("hm_cen", "cen_offset", "direction", "z_coor", "dim", "indices_center", "obj_mask")
LOSS_KEYS = ("total_loss", "hm_cen_loss", "cen_offset_loss", "dim_loss", "direction_loss", "z_coor_loss")
BOUNDARY = {"minX": 0, "maxX": 50, "minY": -25, "maxY": 25, "minZ": -2.73, "maxZ": 1.27}
STATUS_INDEX, STATUS_CLASS = 1, 2


def compute_radius(height: int, width: int, min_overlap: float = 0.7) -> float:
    b1 = height + width
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 + math.sqrt(b1 ** 2 - 4 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    r2 = (b2 + math.sqrt(b2 ** 2 - 16 * c2)) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    r3 = (b3 + math.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def build_targets(labels, hflipped, boundary=BOUNDARY, hm_size=(152, 152), num_classes=3, max_objects=50):
    """One frame.  Returns (targets dict under the reference's keys, status word)."""
    labels = np.asarray(labels, dtype=F).reshape(-1, 8)
    H, W = int(hm_size[0]), int(hm_size[1])
    lo = {k: F(boundary[k]) for k in boundary}
    bsx, bsy = F(boundary["maxX"] - boundary["minX"]), F(boundary["maxY"] - boundary["minY"])
    hm = np.zeros((num_classes, H, W), F)
    cen_offset = np.zeros((max_objects, 2), F)
    direction = np.zeros((max_objects, 2), F)
    z_coor = np.zeros((max_objects, 1), F)
    dim = np.zeros((max_objects, 3), F)
    ind = np.zeros(max_objects, np.int64)
    mask = np.zeros(max_objects, np.uint8)
    status = 0
    ys, xs = np.mgrid[0:H, 0:W]
    for k in range(min(len(labels), max_objects)):
        cf, x, y, z, h, w, l, yaw = (F(v) for v in labels[k])
        yaw = F(-yaw)
        if not (lo["minX"] <= x <= lo["maxX"] and lo["minY"] <= y <= lo["maxY"] and lo["minZ"] <= z <= lo["maxZ"]):
            continue
        if h <= 0 or w <= 0 or l <= 0:
            continue
        if not (F(-num_classes - 2) < cf < F(num_classes)):  # int(cls_id) truncates; NaN fails too
            status |= STATUS_CLASS
            continue
        cls = int(cf)
        bbox_l = F(F(l / bsx) * F(H))
        bbox_w = F(F(w / bsy) * F(W))
        radius = max(0, int(compute_radius(math.ceil(bbox_l), math.ceil(bbox_w))))
        cy = F(F(F(x - lo["minX"]) / bsx) * F(H))
        cx = F(F(F(y - lo["minY"]) / bsy) * F(W))
        if hflipped:
            cx = F(F(F(W) - cx) - F(1))
        cxi, cyi = int(cx), int(cy)
        in_map = 0 <= cxi < W and 0 <= cyi < H
        if not in_map:
            status |= STATUS_INDEX
        sigma = (2 * radius + 1) / 6
        dx, dy = xs - cxi, ys - cyi
        patch = (np.abs(dx) <= radius) & (np.abs(dy) <= radius)
        g = np.exp(-(dx * dx + dy * dy).astype(np.float64) / (2 * sigma * sigma)).astype(F)
        if cls < 0:
            for c in (range(num_classes) if cls == -1 else [-cls - 2]):
                hm[c][patch] = np.maximum(hm[c][patch], g[patch])
                if in_map:
                    hm[c, cyi, cxi] = F(0.9999)
            continue
        hm[cls][patch] = np.maximum(hm[cls][patch], g[patch])
        ind[k] = cyi * W + cxi
        cen_offset[k] = F(cx - F(cxi)), F(cy - F(cyi))
        dim[k] = h, w, l
        im = F(math.sin(float(yaw)))
        direction[k] = (F(-im) if hflipped else im), F(math.cos(float(yaw)))
        z_coor[k] = F(z - lo["minZ"])
        mask[k] = 1
    return dict(zip(KEYS, (hm, cen_offset, direction, z_coor, dim, ind, mask))), status


def build_targets_batch(labels, offsets, hflipped=None, **kw):
    """Frames stacked like the loader's collate; status one word per frame."""
    B = len(offsets) - 1
    flips = [False] * B if hflipped is None else list(hflipped)
    per = [build_targets(labels[offsets[b]:offsets[b + 1]], flips[b], **kw) for b in range(B)]
    return {k: np.stack([t[k] for t, _ in per]) for k in KEYS}, np.array([s for _, s in per], np.uint32)


def sigmoid_clamp(x):
    """utils/torch_utils.py:44-45 in float32 (to make test inputs; the GPU's expf may differ in the last bit)."""
    x = np.asarray(x, F)
    return np.clip(F(1) / (F(1) + np.exp(-x)), F(1e-4), F(1 - 1e-4)).astype(F)


def _gather(feat, ind):
    """_transpose_and_gather_feat: feat (B, c, H, W), ind (B, M) -> (B, M, c)."""
    B, c = feat.shape[:2]
    flat = feat.reshape(B, c, -1)
    return np.stack([flat[b][:, ind[b]].T for b in range(B)])


def balanced_l1(diff, alpha=0.5, gamma=1.5, beta=1.0):
    b = math.exp(gamma / alpha) - 1
    with np.errstate(all="ignore"):
        small = alpha / b * (b * diff + 1) * np.log(b * diff / beta + 1) - alpha * diff
    return np.where(diff < beta, small, gamma * diff + gamma / b - alpha * beta)


def compute_loss(preds, targets):
    """losses.py:138-163 after the two _sigmoid calls: ``preds['hm_cen']`` and ``preds['cen_offset']`` are
    clamped float32 probabilities.  Everything in float64 from the float32 operands.  Returns (the six
    losses in LOSS_KEYS order, the eight raw sums of sfa_compute_loss)."""
    D = np.float64
    p, gt = preds["hm_cen"].astype(D), targets["hm_cen"].astype(D)
    pos_m, neg_m = gt == 1, gt < 1
    pos = float(np.sum((np.log(p) * (1 - p) ** 2)[pos_m]))
    neg = float(np.sum((np.log1p(-p) * p ** 2 * (1 - gt) ** 4)[neg_m]))
    num_pos = float(pos_m.sum())
    hm = -neg if num_pos == 0 else -(pos + neg) / num_pos
    ind = targets["indices_center"]
    m = targets["obj_mask"].astype(D)[:, :, None]

    def masked(key):
        return _gather(preds[key].astype(D), ind) * m, targets[key].astype(D) * m

    s = {}
    for key in ("cen_offset", "direction"):
        a, b = masked(key)
        s[key] = float(np.abs(a - b).sum())
    for key in ("z_coor", "dim"):
        a, b = masked(key)
        s[key] = float(balanced_l1(np.abs(a - b)).sum())
    msum = float(m.sum())
    l_off = s["cen_offset"] / (msum * 2 + 1e-4)
    l_dim = s["dim"] / (msum * 3 + 1e-4)
    l_dir = s["direction"] / (msum * 2 + 1e-4)
    l_z = s["z_coor"] / (msum * 1 + 1e-4)
    total = hm + l_off + l_dim + l_dir + l_z
    return (np.array([total, hm, l_off, l_dim, l_dir, l_z], D),
            np.array([pos, neg, num_pos, s["cen_offset"], s["dim"], s["direction"], s["z_coor"], msum], D))
