"""The FPN neck (models/fpn_resnet.py:197-210) and its gradients restated in numpy float64, with the error bounds the
GPU kernels (csrc/neck_kernel.h) are held to.

Layouts: every map NHWC.  l4 (B, h4, w4, 512), l3 (B, 2 h4, 2 w4, 256), l2 (B, 4 h4, 4 w4, 128), l1 (B, 8 h4, 8 w4,
64); W_f (Cout, Cin_total) and b_f (Cout) of conv_up_level{f}; the first ("up") input columns of W_f are Wfa, the
rest Wfb.  U is the x2 bilinear resize with align_corners=True as upsample2x_bilinear_kernel evaluates it: a
separable matrix whose entries are the float32 values l0 = 1 - l1, l1 = f - floor(f), f = scale * o computed in
float32 with scale = float32(n - 1) / float32(2 n - 1) (0 for n = 1) and the second tap clamped to n - 1.  The
restatement takes those float32 coefficients as exact numbers, so it is the float64 value of the forward that runs.

    z1 = W1 cat(U l4, l3) + b1   u2 = U z1        z2 = W2 cat(u2, l2) + b2   u3 = U z2        u4 = W3 cat(u3, l1) + b3

    dZ3 = g4             dW3 = dZ3^T cat(u3, l1)   db3 = sum dZ3   d_l1 = dZ3 W3b   d_u3 = g3 + dZ3 W3a
    dZ2 = U^T d_u3       dW2 = dZ2^T cat(u2, l2)   db2 = sum dZ2   d_l2 = dZ2 W2b   d_u2 = g2 + dZ2 W2a
    dZ1 = U^T d_u2       dW1b = dZ1^T l3           db1 = sum dZ1   d_l3 = dZ1 W1b
    dL  = U^T dZ1        dW1a = dL^T l4                            d_l4 = dL W1a

Bounds (u = 2^-24, the float32 unit roundoff; r the float64 value of an element; S the same expression on absolute
values).  Every stage is linear with non-negative |coefficients|, so a bound E on the error of a stage's input
passes through the stage as the stage applied to E with |W| (and U, whose entries are non-negative): the
"inherited" term.  Each stage adds its local term:

  dot.  A K-term float32 dot product formed on the f32 MFMA, plus at most one further float32 addition (the bias or
  the g of the map): whatever the order of the additions, each term passes through at most K + 1 roundings, so to
  first order |err| <= (K + 1) u S (Higham, Accuracy and Stability, (3.5)); the test allows (K + 1) u S + u |r| +
  K 2^-126, the last for subnormal products the MFMA may flush.  S is taken on |operand| + E, the magnitudes the
  device really multiplied.
  U.    One output is l0y (l0x a00 + l1x a01) + l1y (l0x a10 + l1x a11) in float32; with or without fused
  multiply-adds a term passes through at most four roundings (product, inner sum, product by the row weight,
  outer sum): 4 u U|x| to first order; the test allows 5 u U|x| for the second-order terms.
  U^T.  At most 25 products coefficient x coefficient x value, each exact or rounded once in float64, added in
  float64 and rounded once to float32: u |r| + 64 2^-53 U^T|x|.
  dW.   Inside one split-K chunk of at most K_c pixels a float32 accumulation: (K_c + 1) u S_chunk; the chunks are
  added in float64 and rounded once: summed over the chunks (K_c + 1) u S + u |r| + chunks 2^-53 S + K 2^-126.
  db.   A float64 sum of n float32 values rounded once: u |r| + n 2^-53 sum|dZ|.

A ratio error / bound above 1 means the kernel or this derivation is wrong; the bound is not to be widened.
"""
import numpy as np

U24 = 2.0 ** -24
U53 = 2.0 ** -53
TINY = 2.0 ** -126
COUT = (256, 128, 64)
UP_C = (512, 256, 128)
SKIP_C = (256, 128, 64)


def up_coeffs(n):
    """Per output index o of the x2 resize of n items: (i0, i1, l0, l1) with the float32 values the kernels compute."""
    one = np.float32(1.0)
    scale = np.float32(n - 1) / np.float32(2 * n - 1) if n > 1 else np.float32(0.0)
    o = np.arange(2 * n, dtype=np.float32)
    f = (scale * o).astype(np.float32)
    i0 = f.astype(np.int32)
    i1 = i0 + (i0 < n - 1)
    l1 = (f - i0.astype(np.float32)).astype(np.float32)
    l0 = (one - l1).astype(np.float32)
    return i0, i1, l0, l1


def up_matrix(n):
    """U of one axis as a float64 (2 n, n) matrix; taps that fall on the same source add."""
    i0, i1, l0, l1 = up_coeffs(n)
    M = np.zeros((2 * n, n))
    rows = np.arange(2 * n)
    np.add.at(M, (rows, i0), l0.astype(np.float64))
    np.add.at(M, (rows, i1), l1.astype(np.float64))
    return M


def up(x):
    """U x: (B, H, W, C) -> (B, 2 H, 2 W, C), float64."""
    x = np.asarray(x, np.float64)
    return np.einsum("yh,xw,bhwc->byxc", up_matrix(x.shape[1]), up_matrix(x.shape[2]), x, optimize=True)


def up_t(g):
    """U^T g: (B, 2 H, 2 W, C) -> (B, H, W, C), float64."""
    g = np.asarray(g, np.float64)
    return np.einsum("yh,xw,byxc->bhwc", up_matrix(g.shape[1] // 2), up_matrix(g.shape[2] // 2), g, optimize=True)


def _f64(*a):
    return [None if v is None else np.asarray(v, np.float64) for v in a]


def _zero(x):
    return np.zeros_like(np.asarray(x, np.float64))


def dot_bound(r, S, K):
    return (K + 1) * U24 * S + U24 * np.abs(r) + K * TINY


def conv(xu, xs, W, b, Eu=None):
    """(z, E): z = W cat(xu, xs) + b per pixel and its bound, Eu the bound on xu's own error (None: exact)."""
    xu, xs, W, b = _f64(xu, xs, W, b)
    ku = xu.shape[-1]
    Wa, Wb = W[:, :ku], W[:, ku:]
    z = xu @ Wa.T + xs @ Wb.T + b
    Eu = _zero(xu) if Eu is None else Eu
    S = (np.abs(xu) + Eu) @ np.abs(Wa).T + np.abs(xs) @ np.abs(Wb).T + np.abs(b)
    return z, dot_bound(z, S, W.shape[1]) + Eu @ np.abs(Wa).T


def up_b(x, E=None):
    """(U x, bound) with E the bound on x's own error."""
    x = np.asarray(x, np.float64)
    E = _zero(x) if E is None else E
    return up(x), up(E) + 5 * U24 * up(np.abs(x) + E)


def up_t_b(g, E=None, f32=False):
    g = np.asarray(g, np.float64)
    E = _zero(g) if E is None else E
    r = up_t(g)
    local = 30 * U24 if f32 else 64 * U53
    return r, up_t(E) + U24 * np.abs(r) + local * up_t(np.abs(g) + E)


def stage1(l4, l3, W1, b1):
    """(u2, E) from the stage's own inputs: U l4, the convolution, the resize of its output."""
    a, Ea = up_b(l4)
    z, Ez = conv(a, l3, W1, b1, Ea)
    return up_b(z, Ez)


def stage2(u2, l2, W2, b2, Eu=None):
    z, Ez = conv(u2, l2, W2, b2, Eu)
    return up_b(z, Ez)


def stage3(u3, l1, W3, b3, Eu=None):
    return conv(u3, l1, W3, b3, Eu)


def forward(l1, l2, l3, l4, params):
    """The whole chain: ((u2, u3, u4), (E2, E3, E4)) with every stage's error carried into the next."""
    W1, b1, W2, b2, W3, b3 = params
    u2, E2 = stage1(l4, l3, W1, b1)
    u3, E3 = stage2(u2, l2, W2, b2, E2)
    u4, E4 = stage3(u3, l1, W3, b3, E3)
    return (u2, u3, u4), (E2, E3, E4)


def _dgrad(dz, Edz, Wseg, g=None):
    """dz Wseg (+ g) per pixel and its bound; Wseg (Cout, n): the segment's columns."""
    r = dz @ Wseg + (0.0 if g is None else g)
    S = (np.abs(dz) + Edz) @ np.abs(Wseg) + (0.0 if g is None else np.abs(g))
    return r, dot_bound(r, S, Wseg.shape[0]) + Edz @ np.abs(Wseg)


def _wgrad(dz, Edz, x, Kc):
    """dz^T x over all pixels and its bound with chunks of at most Kc pixels."""
    n = dz.shape[-1]
    d2, E2, x2 = dz.reshape(-1, n), Edz.reshape(-1, n), x.reshape(-1, x.shape[-1])
    npix = d2.shape[0]
    r = d2.T @ x2
    S = (np.abs(d2) + E2).T @ np.abs(x2)
    chunks = -(-npix // Kc)
    return r, (Kc + 1) * U24 * S + U24 * np.abs(r) + chunks * U53 * S + npix * TINY + E2.T @ np.abs(x2)


def _bgrad(dz, Edz, f32=False):
    n = dz.shape[-1]
    d2, E2 = dz.reshape(-1, n), Edz.reshape(-1, n)
    r = d2.sum(0)
    return r, U24 * np.abs(r) + d2.shape[0] * (U24 if f32 else U53) * (np.abs(d2) + E2).sum(0) + E2.sum(0)


def backward(l1, l2, l3, l4, u2, u3, g2, g3, g4, params, Kc=(None, None, None), f32=False):
    """The ten gradients and their bounds: two dicts with keys d_l1..d_l4, dW1, db1, dW2, db2, dW3, db3 (dW_f (Cout,
    Cin_total)), and a third with the intermediate dZ2, dZ1, dL.  g2 / g3 may be None (zero); Kc = the largest
    split-K chunk of dW1, dW2, dW3 in pixels (None: all pixels in one float32 accumulation).  ``f32``: the bounds of
    an implementation that also forms U^T and the bias sums in float32 in any order (torch on the CPU: the golden
    fixture's reference), where a term of the n-term bias sum passes through at most n roundings and one of the at
    most 25-term U^T sum through at most 30 (25 additions, the products of the coefficients and by the value)."""
    l1, l2, l3, l4, u2, u3, g2, g3, g4 = _f64(l1, l2, l3, l4, u2, u3, g2, g3, g4)
    W1, b1, W2, b2, W3, b3 = _f64(*params)
    kc = [k if k else int(np.prod(m.shape[:3])) for k, m in zip(Kc, (l3, l2, l1))]
    R, E, mid = {}, {}, {}
    dz3, Ez3 = g4, _zero(g4)
    R["d_l1"], E["d_l1"] = _dgrad(dz3, Ez3, W3[:, 128:])
    R["dW3"], E["dW3"] = _wgrad(dz3, Ez3, np.concatenate([u3, l1], -1), kc[2])
    R["db3"], E["db3"] = _bgrad(dz3, Ez3, f32)
    du3, Eu3 = _dgrad(dz3, Ez3, W3[:, :128], g3)
    dz2, Ez2 = up_t_b(du3, Eu3, f32)
    R["d_l2"], E["d_l2"] = _dgrad(dz2, Ez2, W2[:, 256:])
    R["dW2"], E["dW2"] = _wgrad(dz2, Ez2, np.concatenate([u2, l2], -1), kc[1])
    R["db2"], E["db2"] = _bgrad(dz2, Ez2, f32)
    du2, Eu2 = _dgrad(dz2, Ez2, W2[:, :256], g2)
    dz1, Ez1 = up_t_b(du2, Eu2, f32)
    R["d_l3"], E["d_l3"] = _dgrad(dz1, Ez1, W1[:, 512:])
    R["db1"], E["db1"] = _bgrad(dz1, Ez1, f32)
    dwb, Ewb = _wgrad(dz1, Ez1, l3, kc[0])
    dl, El = up_t_b(dz1, Ez1, f32)
    R["d_l4"], E["d_l4"] = _dgrad(dl, El, W1[:, :512])
    dwa, Ewa = _wgrad(dl, El, l4, min(kc[0], int(np.prod(l4.shape[:3]))))
    R["dW1"], E["dW1"] = np.concatenate([dwa, dwb], 1), np.concatenate([Ewa, Ewb], 1)
    mid.update(dZ2=dz2, dZ1=dz1, dL=dl)
    return R, E, mid


def loss(l1, l2, l3, l4, params, g2, g3, g4):
    """<u2, g2> + <u3, g3> + <u4, g4> in float64: what the golden generator backpropagates."""
    (u2, u3, u4), _ = forward(l1, l2, l3, l4, _f64(*params))
    return float((u2 * g2).sum() + (u3 * g3).sum() + (u4 * g4).sum())


def draw_case(B, h4, w4, seed, scale=1.0):
    """Seeded inputs of one shape: (l1, l2, l3, l4) float32 NHWC and (g2, g3, g4)."""
    rng = np.random.default_rng(seed)
    ls = [(scale * rng.standard_normal((B, h4 << (3 - i), w4 << (3 - i), 64 << i))).astype(np.float32) for i in range(4)]
    gs = [rng.standard_normal(s).astype(np.float32) for s in
          ((B, 4 * h4, 4 * w4, 256), (B, 8 * h4, 8 * w4, 128), (B, 8 * h4, 8 * w4, 64))]
    return ls, gs


def draw_params(seed):
    """The six neck parameters at unit scale (rows of about unit norm), float32, torch's 2-D shapes."""
    rng = np.random.default_rng(seed)
    out = []
    for co, cu, cs in zip(COUT, UP_C, SKIP_C):
        out.append((rng.standard_normal((co, cu + cs)) / np.sqrt(cu + cs)).astype(np.float32))
        out.append(rng.standard_normal(co).astype(np.float32))
    return out
