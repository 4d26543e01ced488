"""Restatement of the reference's apply_kfpn (models/fpn_resnet.py:248-254) with the nearest resize of level 0
(:229-230), and of its gradient, for sfa_kfpn_combine / sfa_kfpn_combine_grad.

Forward, every dtype explicit, float32 torch semantics: per element of the three stacked levels
  mx = max(v0, v1, v2);  e_i = exp(v_i - mx);  s = e0 + e1 + e2;  w_i = e_i / s;  out = v0 w0 + v1 w1 + v2 w2
each operation rounded to float32 (torch's softmax subtracts the max, then exp, sum, divide; the product and the
sum over the last axis follow).  numpy's float32 exp may differ from torch's and from the device's expf in the
last bits: the forward is compared through the project's per-kernel gate, not bit for bit.

Gradient, closed form in float64 from the float32 operands.  With w = softmax(v), out = sum_i v_i w_i and
g = d total / d out:  d out / d v_j = w_j + sum_i v_i w_i (delta_ij - w_j) = w_j (1 + v_j - out), so
  d total / d v_j = g w_j (1 + v_j - out).
With level 0 at half resolution, F.interpolate's nearest resize copies cell (y // 2, x // 2) to (y, x); its adjoint
adds the four children's terms into the cell, here in the order (0,0), (0,1), (1,0), (1,1).

Error bound of the device's gradient against grad() (GRAD_REL, GRAD_ABS, GRAD_FLOOR), derived, not measured.
Both sides evaluate the same closed form in float64 from the same float32 operands; u = 2^-53 is the float64 unit
roundoff, V = max_i |v_i|.  Per side:
  * v_i - mx is exact unless the operands' exponents are more than 28 apart; then its relative error u moves
    e_i = exp(x) by |x| e^x u <= u / e absolutely (x <= 0).  exp itself is taken as accurate to 2 ulp, 4 u.
  * w_j = e_j / s: relative error <= 4 u (e_j) + 6 u (s: its terms and two additions) + u, plus 2 u absolute from
    the arguments: <= 12 u w_j + 2 u.
  * out = sum v_i w_i: absolute error <= V (12 u + 2 u + 3 u) sum_i w_i + ... <= 24 u V.
  * t = 1 + v_j - out: absolute error <= 24 u V + 2 u (1 + 2 V) <= 28 u (1 + V);  |t| <= 1 + 2 V <= 2 (1 + V).
  * d = g w_j t: |g| [w_j 28 u (1 + V) + |t| (12 u w_j + 2 u)] + 2 u |d| <= 56 u |g| (1 + V) + 2 u |d|, and
    |d| <= 2 |g| (1 + V), so <= 60 u |g| (1 + V).
  * the gather adds four such terms: 3 u sum_c |d_c| <= 6 u sum_c |g_c| (1 + V_c) more.
Two sides: an absolute part <= 2 (60 + 6) u sum_c |g_c| (1 + V_c) = 66 * 2^-52 sum_c |g_c| (1 + V_c), rounded up to
GRAD_ABS = 80 * 2^-52.  It carries the cancellation in 1 + v_j - out: where t is near 0 the result is far below |g|
and a relative bound alone could not hold.  The device then rounds once to float32: 2^-24 relative, or within one
subnormal step, 2^-149, below the normal range; GRAD_REL adds 4 * 2^-52 (two float64 ulps of exp per side) for the
second-order products of the two parts.
  |device - grad()| <= GRAD_REL |grad()| + GRAD_ABS sum_children |g| (1 + V) + GRAD_FLOOR
Against the reference's float32 autograd the fixture's d_ref = |reference - grad()| is added (triangle inequality).
"""
import numpy as np

F, D = np.float32, np.float64

GRAD_REL = 2.0 ** -24 + 4 * 2.0 ** -52
GRAD_ABS = 80 * 2.0 ** -52
GRAD_FLOOR = 2.0 ** -149  # one float32 subnormal step: the rounding's half step and a flush of the last bit
GATE = 1e-5  # the project's per-kernel gate, <= GATE * max(1, |ref|)


def upsample0(level0, level0_half):
    """F.interpolate(size=(2 h0, 2 w0)) in its default nearest mode at an exact 0.5 scale: src = dst // 2."""
    level0 = np.asarray(level0)
    return level0.repeat(2, axis=2).repeat(2, axis=3) if level0_half else level0


def downsum0(full):
    """The adjoint of upsample0: each (h / 2, w / 2) cell is the sum of its children (0,0), (0,1), (1,0), (1,1)."""
    return ((full[:, :, 0::2, 0::2] + full[:, :, 0::2, 1::2]) + full[:, :, 1::2, 0::2]) + full[:, :, 1::2, 1::2]


def forward(levels, level0_half=False):
    """levels: three float32 arrays (level 0 at half resolution under ``level0_half``).  Returns (out (B, c, h, w),
    weights (B, c, h, w, 3)), float32, every operation rounded to float32."""
    v = np.stack([upsample0(levels[0], level0_half).astype(F), np.asarray(levels[1], F), np.asarray(levels[2], F)], -1)
    mx = v.max(axis=-1, keepdims=True)
    with np.errstate(under="ignore"):
        e = np.exp((v - mx).astype(F)).astype(F)
        s = ((e[..., 0] + e[..., 1]).astype(F) + e[..., 2]).astype(F)
        wts = (e / s[..., None]).astype(F)
        prod = (v * wts).astype(F)
    out = ((prod[..., 0] + prod[..., 1]).astype(F) + prod[..., 2]).astype(F)
    return out, wts


def forward64(levels, level0_half=False):
    """The same map in float64 (the finite-difference check differentiates this one)."""
    v = np.stack([upsample0(levels[0], level0_half).astype(D), np.asarray(levels[1], D), np.asarray(levels[2], D)], -1)
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    wts = e / e.sum(axis=-1, keepdims=True)
    return (v * wts).sum(axis=-1), wts


def grad(levels, g, level0_half=False):
    """d total / d levels in float64, not rounded, from the operands' values: [g0, g1, g2] of the levels' shapes."""
    out, wts = forward64(levels, level0_half)
    v = [upsample0(levels[0], level0_half).astype(D), np.asarray(levels[1], D), np.asarray(levels[2], D)]
    g = np.asarray(g, D)
    with np.errstate(under="ignore"):
        d = [g * wts[..., j] * (1 + v[j] - out) for j in range(3)]
    if level0_half:
        d[0] = downsum0(d[0])
    return d


def grad_bound(levels, g, level0_half=False):
    """Per element of the three gradient maps, the bound of the module docstring without its relative part:
    GRAD_ABS sum_children |g| (1 + V) + GRAD_FLOOR."""
    v = np.stack([np.abs(upsample0(levels[0], level0_half)).astype(D), np.abs(np.asarray(levels[1], D)),
                  np.abs(np.asarray(levels[2], D))], -1)
    a = GRAD_ABS * np.abs(np.asarray(g, D)) * (1 + v.max(axis=-1))
    return [(downsum0(a) if level0_half else a) + GRAD_FLOOR, a + GRAD_FLOOR, a + GRAD_FLOOR]


def within(got, mine, absolute, extra=0.0):
    """|got - mine| <= GRAD_REL |mine| + absolute (+ extra), per element; returns (ok, max error / bound)."""
    err = np.abs(np.asarray(got, D) - mine)
    bound = GRAD_REL * np.abs(mine) + absolute + extra
    return bool(np.all(err <= bound)), float(np.max(err / bound))
