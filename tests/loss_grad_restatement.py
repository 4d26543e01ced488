"""numpy float64 restatement of d total_loss / d (the five head maps) for the reference's Compute_Loss
(losses/losses.py:44-163, unit weights), from the float32 operands: the closed form sfa_compute_loss_grad
evaluates, and what autograd leaves at the heads after ``total_loss.backward()`` (train.py:190-247).

With p the probability of a cell, k = -1 / num_pos (-1 when num_pos == 0; num_pos counts gt == 1 over the
whole batch), m a slot's mask, d = pred m - t m at the slot's cell and S the mask sum:
  hm_cen       gt == 1: k [(1-p)^2 / p - 2 (1-p) log p];  gt < 1: k (1-gt)^4 [2 p log(1-p) - p^2 / (1-p)]
  cen_offset, direction    sign(d) m / (2 S + 1e-4), sign(0) = 0 (torch's l1 backward)
  z_coor, dim              sign(d) m (alpha log(b |d| + 1) if |d| < 1 else gamma) / (c S + 1e-4), c = 1, 3,
                           alpha 0.5, gamma 1.5, b = e^(gamma / alpha) - 1
gather's backward is a scatter-add: the slots of one frame that share a cell add up, here in slot order.
A slot whose index is outside the map contributes nothing and does not count in S (sfa_compute_loss's rule).

``apply_sigmoid``: the hm_cen and cen_offset inputs are logits, ``s`` holds their sigmoid before the clamp,
p = clip(s, f32(1e-4), f32(1 - 1e-4)) and the gradient is taken with respect to the logit: times s (1 - s)
where f32(1e-4) <= s <= f32(1 - 1e-4), both ends included (torch's clamp backward), 0 elsewhere."""
import math

import numpy as np

F, D = np.float32, np.float64
HEADS = ("hm_cen", "cen_offset", "direction", "z_coor", "dim")
LO, HI = F(1e-4), F(1 - 1e-4)
ALPHA, GAMMA = 0.5, 1.5
BB = math.exp(GAMMA / ALPHA) - 1


def np_sigmoid(x):
    """torch's x.sigmoid_() restated in float32 (to make test inputs; a GPU's expf may differ in the last bits)."""
    x = np.asarray(x, F)
    return (F(1) / (F(1) + np.exp(-x))).astype(F)


def chain(s):
    """d clamp(sigmoid(x)) / dx from s = sigmoid(x)."""
    s = np.asarray(s)
    inside = (s >= LO) & (s <= HI)
    s = s.astype(D)
    return np.where(inside, s * (1 - s), 0.0)


def focal_grad(p, gt):
    """d hm_cen_loss / dp, float64, of probabilities p against gt (both (B, C, H, W))."""
    p, gt = np.asarray(p).astype(D), np.asarray(gt).astype(D)
    num_pos = float((gt == 1).sum())
    k = -1.0 if num_pos == 0 else -1.0 / num_pos
    with np.errstate(all="ignore"):
        pos = (1 - p) ** 2 / p - 2 * (1 - p) * np.log(p)
        neg = (1 - gt) ** 4 * (2 * p * np.log1p(-p) - p ** 2 / (1 - p))
    return k * np.where(gt == 1, pos, np.where(gt < 1, neg, 0.0))


def _slope(d, balanced):
    a = np.abs(d)
    if not balanced:
        return np.sign(d)
    return np.sign(d) * np.where(a < 1.0, ALPHA * np.log(BB * a + 1), GAMMA)


def compute_loss_grad(preds, targets, apply_sigmoid=False, s=None):
    """``preds``: the five maps (float32, or float64 for a derivative check).  Without ``apply_sigmoid``
    hm_cen and cen_offset are clamped probabilities; with it they are ignored in favour of ``s`` (a dict with
    the two sigmoid maps before the clamp).  Returns the five gradient maps in float64, not rounded."""
    ind = np.asarray(targets["indices_center"])
    mask = np.asarray(targets["obj_mask"]).astype(D)
    B, M = ind.shape
    prob = {}
    for h in ("hm_cen", "cen_offset"):
        if apply_sigmoid:
            sv = np.asarray(s[h])
            prob[h] = np.clip(sv, LO, HI).astype(D) if sv.dtype == F else np.clip(sv, D(LO), D(HI))
        else:
            prob[h] = np.asarray(preds[h]).astype(D)
    out = {"hm_cen": focal_grad(prob["hm_cen"], targets["hm_cen"])}
    if apply_sigmoid:
        out["hm_cen"] = out["hm_cen"] * chain(s["hm_cen"])
    HW = int(np.prod(out["hm_cen"].shape[2:]))
    live = (mask != 0) & (ind >= 0) & (ind < HW)
    msum = float(mask[live].sum())
    for h, balanced in (("cen_offset", False), ("direction", False), ("z_coor", True), ("dim", True)):
        pred = prob[h] if h in prob else np.asarray(preds[h]).astype(D)
        c = pred.shape[1]
        flat = pred.reshape(B, c, HW)
        g = np.zeros((B, c, HW), D)
        den = msum * c + 1e-4
        t = np.asarray(targets[h]).astype(D)
        fac = chain(s[h]).reshape(B, c, HW) if (apply_sigmoid and h in prob) else None
        for b in range(B):
            for k in range(M):  # slot order
                if not live[b, k]:
                    continue
                i, m = int(ind[b, k]), mask[b, k]
                v = _slope(flat[b, :, i] * m - t[b, k] * m, balanced) * m / den
                if fac is not None:
                    v = v * fac[b, :, i]
                g[b, :, i] += v
        out[h] = g.reshape(pred.shape)
    return out


def ulp_shift(s, n):
    """float32 s moved by n units in the last place."""
    s = np.asarray(s, F).copy()
    for _ in range(abs(n)):
        s = np.nextafter(s, F(np.inf if n > 0 else -np.inf))
    return s


def sigmoid_slack(preds, targets, s, ulps=2):
    """Per element, the largest change of the apply_sigmoid gradient when every s moves by up to ``ulps``
    float32 units in the last place (the accuracy of the device's sigmoid): max over the shifts -ulps..ulps."""
    base = compute_loss_grad(preds, targets, True, s)
    slack = {h: np.zeros_like(v) for h, v in base.items()}
    for n in range(-ulps, ulps + 1):
        if n == 0:
            continue
        moved = compute_loss_grad(preds, targets, True, {h: ulp_shift(v, n) for h, v in s.items()})
        for h in HEADS:
            slack[h] = np.maximum(slack[h], np.abs(moved[h] - base[h]))
    return base, slack
