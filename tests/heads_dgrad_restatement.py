"""The input gradient of one KFPN level's detection heads and the heads' 1x1 output, restated in numpy float64, with
the error bounds the GPU kernels (csrc/heads_grad_kernel.h heads_dgrad_kernel, heads_out_kernel) are held to.

Layouts as tests/heads_grad_restatement.py: x, dX (B, h, w, Cin) NHWC; W1 (O, Cin, 3, 3); dA, Hd (B, h, w, O) with O
the hidden channels of ALL heads of the level side by side (every head reads the same x, so the sum over o runs over
all of them); W2 (c, 64) and b2 (c) per head; y (B, c, h, w).

    dX[b,y,x,i] = sum_o sum_{ky,kx} dA[b, y+1-ky, x+1-kx, o] W1[o,i,ky,kx]       (dA zero outside the map)
    y[b,c,p]    = b2[c] + sum_k W2[c,k] Hd[b,p,k]

With ``shifted`` of the parameter-gradient restatement, dA[b, y+1-ky, x+1-kx] = shifted(dA, 2-ky, 2-kx)[b, y, x].

Bounds (u = 2^-24, the float32 unit roundoff; r the float64 reference of an element):

  dX.  One element is a sum of K = 9 O products of float32 values (fewer at the border: absent taps are exact
  zeros), formed on the f32 MFMA with float32 accumulation, all inside one workgroup.  Whatever the order of the
  additions inside the instruction and across the k-steps, and whether or not a product is rounded before it is
  added, each term passes through at most K roundings (K - 1 additions, + 1 for a product that is not fused), so
  to first order |err| <= K u S with S = sum |dA| |W1| over the element's terms (Higham, Accuracy and Stability,
  (4.4)).  The test allows (9 O + 1) u S + u |r|: the same form as bound_dW1 with K_c = 9 O, the extra u S + u |r|
  covering a final rounding of the stored value, which this kernel does not even need (the accumulator is stored
  as it is).  An MFMA may flush a subnormal product or partial sum: 2^-126 per term at most, the floor bound_dW1
  uses, here 9 O terms.

  y.  65 terms (b2 and 64 products, each exact in float64: 48 significand bits) added in float64 in a fixed order:
  64 additions, |err| <= 64 2^-53 sum|terms| to first order, then one rounding to float32: u |r| + 64 2^-53 sum|terms|.

A ratio error / bound above 1 means the kernel or this derivation is wrong; the bound is not to be widened.
"""
import numpy as np

from heads_grad_restatement import TAPS, U24, shifted


def dgrad(dA, W1):
    """(dX, S) in float64 from the float32 operands: dA (B, h, w, O), W1 (O, Cin, 3, 3); S = sum |dA| |W1|."""
    dA, W1 = np.asarray(dA, np.float64), np.asarray(W1, np.float64)
    B, h, w, O = dA.shape
    C = W1.shape[1]
    dX, S = np.zeros((B, h, w, C)), np.zeros((B, h, w, C))
    for ky, kx in TAPS:
        ds = shifted(dA, 2 - ky, 2 - kx).reshape(-1, O)
        dX += (ds @ W1[:, :, ky, kx]).reshape(dX.shape)
        S += (np.abs(ds) @ np.abs(W1[:, :, ky, kx])).reshape(S.shape)
    return dX, S


def head_out(Hd, W2, b2):
    """(y, sum|terms|) in float64 from a given Hd (B, h, w, 64) of one head: y (B, c, h, w)."""
    Hd = np.asarray(Hd, np.float64)
    b2 = np.asarray(b2, np.float64)
    W2 = np.asarray(W2, np.float64).reshape(len(b2), -1)
    y = np.einsum("bhwo,co->bchw", Hd, W2) + b2[None, :, None, None]
    mag = np.einsum("bhwo,co->bchw", np.abs(Hd), np.abs(W2)) + np.abs(b2)[None, :, None, None]
    return y, mag


def bound_dX(ref, S, O):
    return (9 * O + 1) * U24 * S + U24 * np.abs(ref) + 9 * O * 2.0 ** -126


def bound_y(ref, mag):
    return U24 * np.abs(ref) + 64 * 2.0 ** -53 * mag


def one_hot_case(B, h, w, C, O, b0, y0, x0, o0, seed=0):
    """W1 with all values distinct (and exact in float32) and the dX that a one-hot dA (1.0 at (b0, y0, x0, o0))
    gives: pixel (y, x) takes the tap with y + 1 - ky = y0 and x + 1 - kx = x0, so W1[o0, :, ky, kx] lands at
    (y0 + ky - 1, x0 + kx - 1) where that lies in the map, and everything else is zero, exactly.
    Returns (W1 float32 (O, C, 3, 3), dA float32, dX float32)."""
    rng = np.random.default_rng(seed)
    n = O * C * 9
    W1 = ((rng.permutation(n).astype(np.float32) - 0.5 * n) / 64.0).reshape(O, C, 3, 3)
    dA = np.zeros((B, h, w, O), np.float32)
    dA[b0, y0, x0, o0] = 1.0
    dX = np.zeros((B, h, w, C), np.float32)
    for ky, kx in TAPS:
        yy, xx = y0 + ky - 1, x0 + kx - 1
        if 0 <= yy < h and 0 <= xx < w:
            dX[b0, yy, xx] = W1[o0, :, ky, kx]
    return W1, dA, dX
