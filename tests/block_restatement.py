"""One BasicBlock (models/fpn_resnet.py:42-71) in eval() mode, its gradients and the BatchNorm unfold restated in numpy
float64, with the error bounds the GPU kernels (csrc/block_kernel.h) are held to.

Block layer{L}.{b}: Cout = 64 2^(L-1); for b == 0 and L > 1 stride s = 2, Cin = Cout / 2 and a 1x1 stride-2
downsample, else s = 1, Cin = Cout and the identity skip.  Maps are NHWC: x (B, h, w, Cin); mid, y, gy (B, oh, ow,
Cout), oh = ceil(h / s).  The folded parameters are float32 as the library packs them (csrc/pack_row.h pack_bn_fold,
csrc/pack_host.h): W' = float32(W * scale), scale = gamma / sqrt(var + 1e-5) in float64, rows [o][(kh * 3 + kw) C + c];
b' = float32(beta - mean * scale); with a downsample b2' = float32(shift2 + shift_d).

    a  = ReLU(conv3x3_s(x; W1') + b1')      z = conv3x3_1(a; W2') + b2' + skip      y = ReLU(z)
    dZ = y > 0 ? gy : 0        db2' = sum dZ      dW2' = wgrad_1(dZ, a)       dApost = dgrad_1(dZ; W2')
    dA = a > 0 ? dApost : 0    db1' = sum dA      dW1' = wgrad_s(dA, x)       dWd' = wgrad1x1_s(dZ, x)
    dx = dgrad_s(dA; W1') + (dZ | dgrad1x1_s(dZ; Wd'))
    unfold: dW = s dW',  dbeta = db',  dgamma = (sum_k W dW' - mean db') / sqrt(var + eps)

The gradient is a function of the maps it is given (the masks are read from the mid and y passed in), so gradient
cases draw mid and y themselves, with about half exact zeros, and no test depends on how a forward rounds a
pre-activation near zero.

Bounds (u = 2^-24; r the float64 value; S the same expression on absolute values; E a bound already carried by an
operand, passed through a linear stage as the stage applied to E with |W|: the "inherited" term).  Local terms, as
tests/neck_restatement.py derives them:
  dot.  A K-term float32 MFMA dot product plus at most one further float32 addition (the identity skip's dZ):
        (K + 1) u S + u |r| + K 2^-126.  K = 9 Cout, + Cout with the downsample segment.
  dW.   (K_c + 1) u S + u |r| + chunks 2^-53 S + npix 2^-126 for float32 chunks of at most K_c pixels folded in
        float64 and rounded once.
  sum.  u |r| + n 2^-53 sum|.| for a float64 sum of n terms rounded once (db; dgamma, whose two terms are both
        inside the sum of absolute values, n = K + 2 counting the product, the difference and the division).
  ReLU masks are exact selections: dZ carries no error, dA carries dApost's where mid > 0.
``f32=True`` gives the bounds of the reference: torch on the CPU in float32, the block NOT folded.  It forms every sum
in float32 in any order, so a term of an n-term sum passes through at most n roundings: K_c = npix in dW and n u
instead of n 2^-53 in sums.  It also reaches the same numbers by another route, conv(x; W) then the BatchNorm's affine
map, where the restatement multiplies by W' = float32(s W).  Per term that route adds at most REF_EXTRA = 8 roundings
to either side: the BatchNorm's scale in float32 (var + eps, the square root, the division, the product with gamma:
4), the product of the gradient with that scale (1), the product inside the convolution (1), and on the restatement's
side the rounding of W' and of b' (2).  So every K + 1 becomes K + 1 + REF_EXTRA.  The reference's dgamma is
sum_p dY (conv(x; W) - mean) / sd: a term passes through the convolution's K roundings, the npix of the pixel sum and
the 8: (K + npix + 8) u S_gamma + u |r|, S_gamma = (sum_k |W| S_dW' + |mean| S_db') / sd with S_dW' = |dY|^T |patches|
and S_db' = sum |dY|, the sums of absolute terms behind dW' and db' (backward() returns them as E["S:..."]).

A ratio error / bound above 1 means the kernel or this derivation is wrong; the bound is not to be widened.
"""
import numpy as np

U24 = 2.0 ** -24
U53 = 2.0 ** -53
TINY = 2.0 ** -126
EPS = 1e-5
GRADS = ("dx", "dW1", "db1", "dW2", "db2", "dWd")


def block_shape(layer, block):
    """(Cin, Cout, stride, has_downsample)."""
    cout = 64 << (layer - 1)
    ds = block == 0 and layer > 1
    return (cout // 2 if ds else cout), cout, (2 if ds else 1), ds


def draw_params(layer, block, seed):
    """Raw parameters of the block, float32, torch's shapes: {conv1, bn1, conv2, bn2[, convd, bnd]} with bn =
    (gamma, beta, mean, var)."""
    cin, cout, _, ds = block_shape(layer, block)
    rng = np.random.default_rng(seed)

    def conv(co, ci, k):
        return (rng.standard_normal((co, ci, k, k)) / np.sqrt(9 * ci)).astype(np.float32)

    def bn(c):
        return (rng.uniform(0.5, 1.5, c).astype(np.float32), (0.3 * rng.standard_normal(c)).astype(np.float32),
                (0.3 * rng.standard_normal(c)).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32))

    p = dict(conv1=conv(cout, cin, 3), bn1=bn(cout), conv2=conv(cout, cout, 3), bn2=bn(cout))
    if ds:
        p["convd"], p["bnd"] = conv(cout, cin, 1), bn(cout)
    return p


def state_entries(layer, block, p):
    """The block's state-dict entries {name: array}."""
    pre = f"layer{layer}.{block}"
    out = {}
    for conv, bn, cn, bnn in (("conv1", "bn1", "conv1", "bn1"), ("conv2", "bn2", "conv2", "bn2"),
                              ("convd", "bnd", "downsample.0", "downsample.1")):
        if conv not in p:
            continue
        out[f"{pre}.{cn}.weight"] = p[conv]
        for k, n in zip(p[bn], ("weight", "bias", "running_mean", "running_var")):
            out[f"{pre}.{bnn}.{n}"] = k
    return out


def _fold_one(w, bn):
    g, b, mu, var = (np.asarray(v, np.float64) for v in bn)
    scale = g / np.sqrt(var + EPS)
    W = (np.asarray(w, np.float64) * scale[:, None, None, None]).astype(np.float32)
    return W.transpose(0, 2, 3, 1).reshape(w.shape[0], -1), b - mu * scale


def fold(p):
    """The float32 folded parameters as the library packs them: W1 (Cout, 9 Cin), b1, W2 (Cout, 9 Cout), b2, Wd (Cout,
    Cin) or None."""
    W1, s1 = _fold_one(p["conv1"], p["bn1"])
    W2, s2 = _fold_one(p["conv2"], p["bn2"])
    Wd = None
    if "convd" in p:
        Wd, sd = _fold_one(p["convd"], p["bnd"])
        b2 = (s2 + sd).astype(np.float32)
    else:
        b2 = s2.astype(np.float32)
    return dict(W1=W1, b1=s1.astype(np.float32), W2=W2, b2=b2, Wd=Wd)


def patches(x, s):
    """(B, oh, ow, 9, C): the 3x3 / pad 1 / stride s windows of x (B, h, w, C), zero outside."""
    x = np.asarray(x, np.float64)
    B, h, w, C = x.shape
    oh, ow = -(-h // s), -(-w // s)
    xp = np.zeros((B, s * (oh - 1) + 3, s * (ow - 1) + 3, C))  # index i + 1; x always fits: h <= s (oh - 1) + 2
    xp[:, 1:h + 1, 1:w + 1] = x
    out = np.empty((B, oh, ow, 9, C))
    for ky in range(3):
        for kx in range(3):
            out[:, :, :, ky * 3 + kx] = xp[:, ky:ky + s * (oh - 1) + 1:s, kx:kx + s * (ow - 1) + 1:s]
    return out


def patches_t(cols, s, h, w):
    """The adjoint of patches(): cols (B, oh, ow, 9, C) -> (B, h, w, C)."""
    B, oh, ow, _, C = cols.shape
    xp = np.zeros((B, s * (oh - 1) + 3, s * (ow - 1) + 3, C))
    for ky in range(3):
        for kx in range(3):
            xp[:, ky:ky + s * (oh - 1) + 1:s, kx:kx + s * (ow - 1) + 1:s] += cols[:, :, :, ky * 3 + kx]
    return xp[:, 1:h + 1, 1:w + 1]


def conv3(x, W, s):
    """conv3x3 / pad 1 / stride s of x with W (Cout, 9 C) in float64."""
    c = patches(x, s)
    return c.reshape(c.shape[:3] + (-1,)) @ np.asarray(W, np.float64).T


def dgrad3(g, W, s, h, w):
    """The adjoint of conv3 in x: g (B, oh, ow, Cout) -> (B, h, w, C)."""
    W = np.asarray(W, np.float64)
    cols = np.asarray(g, np.float64) @ W
    return patches_t(cols.reshape(g.shape[:3] + (9, W.shape[1] // 9)), s, h, w)


def forward(x, f, s):
    """(mid, y) in float64 from the float32 folded parameters."""
    x = np.asarray(x, np.float64)
    a = np.maximum(conv3(x, f["W1"], s) + f["b1"].astype(np.float64), 0.0)
    skip = x if f["Wd"] is None else x[:, ::s, ::s] @ f["Wd"].astype(np.float64).T
    return a, np.maximum(conv3(a, f["W2"], 1) + f["b2"].astype(np.float64) + skip, 0.0)


REF_EXTRA = 8  # roundings per term the unfolded float32 reference may add (module docstring)


def dot_bound(r, S, K, extra=0):
    return (K + 1 + extra) * U24 * S + U24 * np.abs(r) + K * TINY


def _wgrad(dz, Edz, cols, Kc, f32):
    """dz^T cols over all pixels: (Cout, taps * C), its bound, and the sum of absolute terms."""
    d2, E2, x2 = dz.reshape(-1, dz.shape[-1]), Edz.reshape(-1, dz.shape[-1]), cols.reshape(-1, int(np.prod(cols.shape[3:])))
    npix = d2.shape[0]
    kc = npix if (f32 or not Kc) else min(Kc, npix)
    r = d2.T @ x2
    S = (np.abs(d2) + E2).T @ np.abs(x2)
    chunks = -(-npix // kc)
    extra = REF_EXTRA if f32 else 0
    return r, (kc + 1 + extra) * U24 * S + U24 * np.abs(r) + chunks * U53 * S + npix * TINY + E2.T @ np.abs(x2), S


def _bgrad(dz, Edz, f32):
    d2, E2 = dz.reshape(-1, dz.shape[-1]), Edz.reshape(-1, dz.shape[-1])
    r = d2.sum(0)
    S = (np.abs(d2) + E2).sum(0)
    return r, U24 * np.abs(r) + (d2.shape[0] + REF_EXTRA if f32 else d2.shape[0]) * (U24 if f32 else U53) * S + E2.sum(0), S


def _torch_w(r, cout, taps):
    """(Cout, taps * C) in (tap, c) order -> torch's (Cout, C, k, k)."""
    k = 3 if taps == 9 else 1
    return r.reshape(cout, k, k, -1).transpose(0, 3, 1, 2)


def backward(x, mid, y, gy, f, s, Kc=None, f32=False):
    """(R, E): the gradients and their bounds, dicts over GRADS (dWd None without a downsample); dW in torch's
    layouts.  Kc: the largest split-K chunk in output pixels (None: all pixels in one float32 accumulation).  E also
    holds, under "S:dW1", "S:db1", ..., the sums of absolute terms behind the parameter gradients."""
    x, mid, y, gy = (np.asarray(v, np.float64) for v in (x, mid, y, gy))
    W1, W2 = f["W1"].astype(np.float64), f["W2"].astype(np.float64)
    B, h, w, cin = x.shape
    cout = W1.shape[0]
    R, E = {}, {}
    dz = np.where(y > 0, gy, 0.0)
    z0 = np.zeros_like(dz)
    extra = REF_EXTRA if f32 else 0
    R["db2"], E["db2"], E["S:db2"] = _bgrad(dz, z0, f32)
    r, e, sm = _wgrad(dz, z0, patches(mid, 1), Kc, f32)
    R["dW2"], E["dW2"], E["S:dW2"] = _torch_w(r, cout, 9), _torch_w(e, cout, 9), _torch_w(sm, cout, 9)
    oh, ow = dz.shape[1:3]
    dap = dgrad3(dz, W2, 1, oh, ow)
    Eap = dot_bound(dap, dgrad3(np.abs(dz), np.abs(W2), 1, oh, ow), 9 * cout, extra)
    da, Eda = np.where(mid > 0, dap, 0.0), np.where(mid > 0, Eap, 0.0)
    R["db1"], E["db1"], E["S:db1"] = _bgrad(da, Eda, f32)
    r, e, sm = _wgrad(da, Eda, patches(x, s), Kc, f32)
    R["dW1"], E["dW1"], E["S:dW1"] = _torch_w(r, cout, 9), _torch_w(e, cout, 9), _torch_w(sm, cout, 9)
    dx = dgrad3(da, W1, s, h, w)
    S = dgrad3(np.abs(da) + Eda, np.abs(W1), s, h, w)
    inh = dgrad3(Eda, np.abs(W1), s, h, w)
    K = 9 * cout
    if f["Wd"] is None:
        dx, S = dx + dz, S + np.abs(dz)
        R["dWd"] = E["dWd"] = None
    else:
        Wd = f["Wd"].astype(np.float64)
        sk, Ssk = np.zeros_like(dx), np.zeros_like(dx)
        sk[:, ::s, ::s] = dz @ Wd
        Ssk[:, ::s, ::s] = np.abs(dz) @ np.abs(Wd)
        dx, S, K = dx + sk, S + Ssk, K + cout
        r, e, sm = _wgrad(dz, z0, x[:, ::s, ::s][:, :, :, None, :], Kc, f32)
        R["dWd"], E["dWd"], E["S:dWd"] = _torch_w(r, cout, 1), _torch_w(e, cout, 1), _torch_w(sm, cout, 1)
    R["dx"], E["dx"] = dx, dot_bound(dx, S, K, extra) + inh
    return R, E


def bn_unfold(W, bn, dWf, dbf, EdW=None, Edb=None, eps=EPS, f32=False, SdW=None, Sdb=None, npix=0):
    """((dW, dgamma, dbeta), bounds) of the raw convolution weight W (Cout, ...) and its BatchNorm from the folded
    gradients dWf (W's shape) and dbf, EdW / Edb the bounds those carry.  ``f32``: the reference's form (module
    docstring), which needs SdW / Sdb, the sums of absolute terms behind dWf / dbf, and the pixel count of those sums."""
    W, dWf, dbf = (np.asarray(v, np.float64) for v in (W, dWf, dbf))
    g, _, mu, var = (np.asarray(v, np.float64) for v in bn)
    EdW = np.zeros_like(dWf) if EdW is None else EdW
    Edb = np.zeros_like(dbf) if Edb is None else Edb
    ax = tuple(range(1, W.ndim))
    sd = np.sqrt(var + eps)
    sc = (g / sd).reshape((-1,) + (1,) * (W.ndim - 1))
    dW = sc * dWf
    K = int(np.prod(W.shape[1:]))
    dg = ((W * dWf).sum(ax) - mu * dbf) / sd
    inh = ((np.abs(W) * EdW).sum(ax) + np.abs(mu) * Edb) / sd
    if f32:
        Sg = ((np.abs(W) * (SdW + EdW)).sum(ax) + np.abs(mu) * (Sdb + Edb)) / sd
        return (dW, dg, dbf), (U24 * np.abs(dW) + np.abs(sc) * EdW,  # EdW already holds the REF_EXTRA roundings
                               U24 * np.abs(dg) + (K + npix + REF_EXTRA) * U24 * Sg + inh, Edb)
    Sg = ((np.abs(W) * (np.abs(dWf) + EdW)).sum(ax) + np.abs(mu) * (np.abs(dbf) + Edb)) / sd
    return (dW, dg, dbf), (U24 * np.abs(dW) + 4 * U53 * np.abs(dW) + np.abs(sc) * EdW,
                           U24 * np.abs(dg) + (K + 2) * U53 * Sg + inh, Edb)


PAIRS = (("conv1", "bn1", "dW1", "db1"), ("conv2", "bn2", "dW2", "db2"), ("convd", "bnd", "dWd", "db2"))


def unfolded(layer, block, p, maps, Kc=None, f32=False):
    """(R, E) keyed "dx", "conv1.weight", "bn1.weight", "bn1.bias", ...: backward() on maps = {x, mid, y, gy} with the
    folded form of the raw parameters p, then bn_unfold() per convolution with the bounds carried through: what
    autograd leaves at x and at the block's 6 or 9 parameters."""
    _, _, s, _ = block_shape(layer, block)
    Rf, Ef = backward(maps["x"], maps["mid"], maps["y"], maps["gy"], fold(p), s, Kc=Kc, f32=f32)
    npix = int(np.prod(np.shape(maps["gy"])[:3]))
    R, E = {"dx": Rf["dx"]}, {"dx": Ef["dx"]}
    for conv, bn, dw, db in PAIRS:
        if conv not in p:
            continue
        rs, es = bn_unfold(p[conv], p[bn], Rf[dw], Rf[db], Ef[dw], Ef[db], f32=f32, SdW=Ef["S:" + dw], Sdb=Ef["S:" + db],
                           npix=npix)
        for k, r, e in zip((conv + ".weight", bn + ".weight", bn + ".bias"), rs, es):
            R[k], E[k] = r, e
    return R, E


def ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is zero (a sum with no non-zero term) the error has to be zero too."""
    err = np.abs(np.asarray(got, np.float64).reshape(np.shape(ref)) - ref)
    bound = np.broadcast_to(bound, err.shape)
    q = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(np.max(q))


def _half_zero(rng, shape, relu=False):
    v = rng.standard_normal(shape)
    v = np.abs(v) if relu else v
    return np.where(rng.random(shape) < 0.5, 0.0, v).astype(np.float32)


def draw_case(layer, block, B, h, w, seed):
    """Seeded maps of one shape, float32 NHWC: x, gy (about half exact zeros), and the mid and y of a gradient-only
    case (non-negative, about half exact zeros)."""
    cin, cout, s, _ = block_shape(layer, block)
    rng = np.random.default_rng(seed)
    osh = (B, -(-h // s), -(-w // s), cout)
    return dict(x=rng.standard_normal((B, h, w, cin)).astype(np.float32), gy=_half_zero(rng, osh),
                mid=_half_zero(rng, osh, True), y=_half_zero(rng, osh, True))
