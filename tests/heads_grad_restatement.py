"""The detection heads of one KFPN level and their parameter gradients, restated in numpy float64
(models/fpn_resnet.py:135-143: conv3x3 -> ReLU -> conv1x1 per head), and the error bounds the GPU kernels
(csrc/heads_grad_kernel.h) are held to.

Layouts: x (B, h, w, Cin) NHWC; W1 (O, Cin, 3, 3), b1 (O), W2 (c, O) or (c, O, 1, 1), b2 (c): torch's own;
A, Hd, dA (B, h, w, O); y, g (B, c, h, w).  O is generic (64 in the model, 8 or 16 in the CPU fixture).

    A = conv3x3(x; W1) + b1        Hd = max(A, 0)        y = W2 Hd + b2
    db2[c]    = sum_{b,p} g[b,c,p]
    dW2[c,o]  = sum_{b,p} g[b,c,p] Hd[b,p,o]
    dA[b,p,o] = Hd[b,p,o] > 0 ? sum_c W2[c,o] g[b,c,p] : 0          (strict, torch's ReLU backward)
    db1[o]    = sum_{b,p} dA[b,p,o]
    dW1[o,i,ky,kx] = sum_{b,y,x} dA[b,y,x,o] x[b,y+ky-1,x+kx-1,i]   (zero outside the map)

The device rounds dA to float32 once and forms db1 and dW1 from the rounded values; so does grads().

Bounds (u = 2^-24, the float32 unit roundoff; r the float64 reference of an element):

  dA.  The device evaluates the <= 4-term sum in float64 and rounds once to float32: |err| <= u |r| plus the
  float64 error of four products and three additions, below 8 * 2^-53 * sum|terms|, which only matters when
  it moves the float32 rounding by one more unit in the last place: 2 u |r| = 2^-23 |r| covers both.

  float64-folded sums (dW2, db1, db2).  n terms, each an exact float32 value or a product of two float32
  values (48 significand bits: exact in float64), added in float64 in some fixed order: the sum of n terms
  carries at most (n - 1) roundings, |err| <= n 2^-53 sum|terms| (Higham, Accuracy and Stability, (4.4), first
  order), then one rounding to float32: 2^-24 |r| + n 2^-53 sum|terms|.

  dW1.  Inside one split-K chunk of at most K_c pixels the products dA x are added on the f32 MFMA: whatever
  the order inside the instruction and across the k-steps, a sum of K terms whose products may be rounded
  separately carries at most K roundings per term, |err_chunk| <= K u S_chunk to first order with S_chunk =
  sum|dA||x| over the chunk ((4.4) again: the constant K - 1 for the additions, + 1 for a product that is
  not fused).  The chunks' float32 results are then added in float64 (exact to 2^-53, absorbed by the + 1)
  and the total is rounded to float32 once: |err| <= (K_c + 1) u S + u |r|, S over all pixels.  An MFMA may
  flush a subnormal product or partial sum: one 2^-126 per term at most, the floor.

A ratio error / bound above 1 means the kernel or this derivation is wrong; the bound is not to be widened.
"""
import numpy as np

U24 = 2.0 ** -24
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def shifted(x, ky, kx):
    """xs[b, y, x_, i] = x[b, y + ky - 1, x_ + kx - 1, i], zero outside the map."""
    B, h, w, C = x.shape
    pad = np.zeros((B, h + 2, w + 2, C), x.dtype)
    pad[:, 1:h + 1, 1:w + 1] = x
    return pad[:, ky:ky + h, kx:kx + w]


def forward(x, W1, b1, W2, b2):
    """(A, Hd, y) in float64 from the float32 operands."""
    x = np.asarray(x, np.float64)
    W1, b1 = np.asarray(W1, np.float64), np.asarray(b1, np.float64)
    W2 = np.asarray(W2, np.float64).reshape(len(b2), -1)
    A = np.zeros(x.shape[:3] + (W1.shape[0],)) + b1
    for ky, kx in TAPS:
        A += (shifted(x, ky, kx).reshape(-1, x.shape[3]) @ W1[:, :, ky, kx].T).reshape(A.shape)
    Hd = np.maximum(A, 0.0)
    y = np.einsum("bhwo,co->bchw", Hd, W2) + np.asarray(b2, np.float64)[None, :, None, None]
    return A, Hd, y


def dhidden(Hd, W2, g):
    """dA in float64 (not yet rounded) and sum_c |W2 g| per element."""
    Hd, g = np.asarray(Hd, np.float64), np.asarray(g, np.float64)
    W2 = np.asarray(W2, np.float64).reshape(g.shape[1], -1)
    mask = Hd > 0
    dA = np.where(mask, np.einsum("co,bchw->bhwo", W2, g), 0.0)
    mag = np.where(mask, np.einsum("co,bchw->bhwo", np.abs(W2), np.abs(g)), 0.0)
    return dA, mag


def grads(x, Hd, W2, g, dA32=None):
    """The five gradients in float64 from the float32 operands, dA rounded to float32 before db1 and dW1 (or
    ``dA32`` given: the device's own).  Returns a dict with dA (float64), dA32, dW1, db1, dW2, db2 and the
    magnitude sums S_* = sum|terms| of dW1, db1, dW2, db2."""
    x, Hd, g = np.asarray(x, np.float64), np.asarray(Hd, np.float64), np.asarray(g, np.float64)
    dA, _ = dhidden(Hd, W2, g)
    if dA32 is None:
        dA32 = dA.astype(np.float32)
    d = np.asarray(dA32, np.float64)
    O, C = d.shape[3], x.shape[3]
    dW1, S1 = np.zeros((O, C, 3, 3)), np.zeros((O, C, 3, 3))
    for ky, kx in TAPS:
        xs = shifted(x, ky, kx)
        xs = xs.reshape(-1, C)
        dW1[:, :, ky, kx] = d.reshape(-1, O).T @ xs
        S1[:, :, ky, kx] = np.abs(d).reshape(-1, O).T @ np.abs(xs)
    return {"dA": dA, "dA32": np.asarray(dA32, np.float32), "dW1": dW1, "S_dW1": S1,
            "db1": d.sum((0, 1, 2)), "S_db1": np.abs(d).sum((0, 1, 2)),
            "dW2": np.einsum("bchw,bhwo->co", g, Hd), "S_dW2": np.einsum("bchw,bhwo->co", np.abs(g), np.abs(Hd)),
            "db2": g.sum((0, 2, 3)), "S_db2": np.abs(g).sum((0, 2, 3))}


def bound_dA(ref):
    return 2.0 * U24 * np.abs(ref)


def bound_f64_sum(ref, S, n):
    return U24 * np.abs(ref) + n * 2.0 ** -53 * S


def bound_dW1(ref, S, Kc, npix):
    return (Kc + 1) * U24 * S + U24 * np.abs(ref) + npix * 2.0 ** -126


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 = 0: an exact element of a zero bound)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max()) if q.size else 0.0


def gate(got, ref, tol=1e-5):
    """The per-kernel parity gate: max |got - ref| / max(1, |ref|) and whether it is <= tol."""
    ref = np.asarray(ref, np.float64)
    q = np.abs(np.asarray(got, np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    worst = float(q.max()) if q.size else 0.0
    return worst, worst <= tol


def one_hot_case(B, h, w, C, O, b0, y0, x0, o0, seed=0):
    """x with all values distinct and the dW1 that a one-hot dA (1.0 at (b0, y0, x0, o0)) gives: a shifted copy
    of x, exactly.  Returns (x float32, dA float32, dW1 float32 (O, C, 3, 3))."""
    rng = np.random.default_rng(seed)
    x = (rng.permutation(B * h * w * C).astype(np.float32) - 0.5 * B * h * w * C).reshape(B, h, w, C) / 64.0
    dA = np.zeros((B, h, w, O), np.float32)
    dA[b0, y0, x0, o0] = 1.0
    dW1 = np.zeros((O, C, 3, 3), np.float32)
    for ky, kx in TAPS:
        yy, xx = y0 + ky - 1, x0 + kx - 1
        if 0 <= yy < h and 0 <= xx < w:
            dW1[o0, :, ky, kx] = x[b0, yy, xx]
    return x, dA, dW1
