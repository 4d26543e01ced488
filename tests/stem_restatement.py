"""The stem of fpn_resnet_18 (models/fpn_resnet.py:179-182: conv1 7x7 / 2 / pad 3 without bias, bn1, ReLU,
MaxPool2d(3, 2, 1)) in eval() mode, its gradients and the BatchNorm unfold restated in numpy float64, with the error
bounds the GPU kernels (csrc/stem_grad_kernel.h) are held to.  Nothing here imports from sfa/.

x is (B, 3, H, W) NCHW; a (B, oh, ow, 64) and p, gp (B, ph, pw, 64) are NHWC, oh = ceil(H / 2), ph = ceil(oh / 2).  The
folded parameters are float32 as the library packs them: W' = float32(W * scale), scale = gamma / sqrt(var + 1e-5) in
float64, b' = float32(beta - mean * scale).

    a   = ReLU(conv7x7_2(x; W') + b')          p = maxpool3x3_2(a)
    dAp = pool adjoint of gp                   dA = a > 0 ? dAp : 0
    db' = sum dA       dW' = wgrad_2(dA, x) (64, 3, 7, 7)       dx = dgrad_2(dA; W')
    unfold (block_restatement.bn_unfold): dW = s dW', dbeta = db', dgamma = (sum_k W dW' - mean db') / sqrt(var + eps)

The first-maximum rule, written out (pool_argmax): a window's nine cells are scanned in row-major order, cells outside
the map are skipped (torch pads with -inf, which never wins), and a cell replaces the running maximum only when it is
strictly larger; so of equal maxima the first in scan order wins and receives the whole of the window's gp.  A cell
of a lies in at most four windows and dAp sums what it wins.

Bounds (u = 2^-24; r the float64 value; S the same expression on absolute values; block_restatement has the local
forms).  dA: the device adds at most four float32 terms, dA = fl(sum): E_dA = 3 u sum|gp won|, carried by every
consumer as an inherited term (the consumer applied to E_dA with absolute operands) and inside its S.
  dW'.  (K_c + 1) u S + u |r| + chunks 2^-53 S + npix 2^-126 (float32 MFMA chunks of at most K_c pixels, folded in
        float64, rounded once).
  db'.  u |r| + n 2^-53 sum|.| (float64 sum of n = npix terms, rounded once).
  dx.   float64 accumulation of exact float32 products, at most n = 16 taps x 64 channels terms, rounded once:
        u |r| + n 2^-53 S.
``f32=True`` gives the bounds of the reference (torch on the CPU in float32, the stem not folded), as
block_restatement derives them: K_c = npix in dW', n u instead of n 2^-53 in sums, REF_EXTRA further roundings per term,
and dx as an n-term float32 dot product, (n + 1 + REF_EXTRA) u S + u |r|.

A ratio error / bound above 1 means the kernel or this derivation is wrong; the bound is not to be widened.
"""
import numpy as np

import block_restatement as br

U24, U53, TINY, EPS = br.U24, br.U53, br.TINY, br.EPS
DX_TERMS = 16 * 64
GRADS = ("dx", "dW", "db")
MARGIN = 1e-3


def draw_params(seed):
    """conv1.weight (64, 3, 7, 7) and bn1 = (gamma, beta, running_mean, running_var), float32, drawn statistics."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((64, 3, 7, 7)) / np.sqrt(147.0)).astype(np.float32)
    bn = (rng.uniform(0.5, 1.5, 64).astype(np.float32), (0.3 * rng.standard_normal(64)).astype(np.float32),
          (0.3 * rng.standard_normal(64)).astype(np.float32), rng.uniform(0.5, 1.5, 64).astype(np.float32))
    return dict(conv1=w, bn1=bn)


def fold(p):
    """(W' (64, 3, 7, 7) float32, b' (64,) float32) as the library packs them."""
    g, b, mu, var = (np.asarray(v, np.float64) for v in p["bn1"])
    scale = g / np.sqrt(var + EPS)
    return ((np.asarray(p["conv1"], np.float64) * scale[:, None, None, None]).astype(np.float32),
            (b - mu * scale).astype(np.float32))


def sizes(H, W):
    oh, ow = -(-H // 2), -(-W // 2)
    return oh, ow, -(-oh // 2), -(-ow // 2)


def patches(x):
    """(B, oh, ow, 147): the 7x7 / pad 3 / stride 2 windows of x (B, 3, H, W) in (c, ky, kx) order, zero outside."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    oh, ow, _, _ = sizes(H, W)
    xp = np.zeros((B, C, 2 * (oh - 1) + 7, 2 * (ow - 1) + 7))  # index i + 3
    xp[:, :, 3:H + 3, 3:W + 3] = x
    out = np.empty((B, oh, ow, C, 7, 7))
    for ky in range(7):
        for kx in range(7):
            out[:, :, :, :, ky, kx] = xp[:, :, ky:ky + 2 * (oh - 1) + 1:2, kx:kx + 2 * (ow - 1) + 1:2].transpose(0, 2, 3, 1)
    return out.reshape(B, oh, ow, C * 49)


def patches_t(cols, H, W):
    """The adjoint of patches(): cols (B, oh, ow, 147) -> (B, 3, H, W)."""
    B, oh, ow, _ = cols.shape
    c6 = cols.reshape(B, oh, ow, 3, 7, 7)
    xp = np.zeros((B, 3, 2 * (oh - 1) + 7, 2 * (ow - 1) + 7))
    for ky in range(7):
        for kx in range(7):
            xp[:, :, ky:ky + 2 * (oh - 1) + 1:2, kx:kx + 2 * (ow - 1) + 1:2] += c6[:, :, :, :, ky, kx].transpose(0, 3, 1, 2)
    return xp[:, :, 3:H + 3, 3:W + 3]


def conv7(x, Wf):
    return patches(x) @ np.asarray(Wf, np.float64).reshape(64, 147).T


def dgrad7(g, Wf, H, W):
    return patches_t(np.asarray(g, np.float64) @ np.asarray(Wf, np.float64).reshape(64, 147), H, W)


def pool_argmax(a):
    """(pooled, arg): per window the maximum and the scan index 3 dy + dx of its FIRST maximum (module docstring)."""
    a = np.asarray(a, np.float64)
    B, oh, ow, C = a.shape
    ph, pw = -(-oh // 2), -(-ow // 2)
    best = np.full((B, ph, pw, C), -np.inf)
    arg = np.full((B, ph, pw, C), -1, np.int64)
    ap = np.full((B, 2 * ph + 1, 2 * pw + 1, C), -np.inf)  # index i + 1
    ap[:, 1:oh + 1, 1:ow + 1] = a
    for dy in range(3):
        for dx in range(3):
            v = ap[:, dy:dy + 2 * ph:2, dx:dx + 2 * pw:2]
            upd = v > best  # strict: an equal later cell does not replace the first; -inf padding never wins
            best = np.where(upd, v, best)
            arg = np.where(upd, 3 * dy + dx, arg)
    return best, arg


def pool_adjoint(a, gp):
    """(dAp, dAp_abs): gp (and |gp|) sent to each window's first maximum, summed over the windows a cell wins."""
    a, gp = np.asarray(a, np.float64), np.asarray(gp, np.float64)
    B, oh, ow, C = a.shape
    _, arg = pool_argmax(a)
    ph, pw = arg.shape[1:3]
    out = np.zeros((2, B, 2 * ph + 1, 2 * pw + 1, C))
    for dy in range(3):
        for dx in range(3):
            won = arg == 3 * dy + dx
            out[0, :, dy:dy + 2 * ph:2, dx:dx + 2 * pw:2] += np.where(won, gp, 0.0)
            out[1, :, dy:dy + 2 * ph:2, dx:dx + 2 * pw:2] += np.where(won, np.abs(gp), 0.0)
    return out[0, :, 1:oh + 1, 1:ow + 1], out[1, :, 1:oh + 1, 1:ow + 1]


def forward(x, Wf, bf):
    """(a, pooled) in float64 from the float32 folded parameters."""
    a = np.maximum(conv7(x, Wf) + np.asarray(bf, np.float64), 0.0)
    return a, pool_argmax(a)[0]


def backward(x, a, gp, Wf, Kc=None, f32=False):
    """(R, E): dx (B, 3, H, W), dW (64, 3, 7, 7), db (64,) and their bounds from the maps given (the masks and the
    window maxima are read from ``a``).  R also holds "dA"; E holds "S:dW", "S:db" (sums of absolute terms)."""
    x, a = np.asarray(x, np.float64), np.asarray(a, np.float64)
    H, W = x.shape[2:]
    dap, dabs = pool_adjoint(a, gp)
    da, Eda = np.where(a > 0, dap, 0.0), np.where(a > 0, 3 * U24 * dabs, 0.0)
    R, E = {"dA": da}, {"dA": Eda}
    R["db"], E["db"], E["S:db"] = br._bgrad(da, Eda, f32)
    r, e, sm = br._wgrad(da, Eda, patches(x), Kc, f32)
    R["dW"], E["dW"], E["S:dW"] = (v.reshape(64, 3, 7, 7) for v in (r, e, sm))
    dx = dgrad7(da, Wf, H, W)
    S = dgrad7(np.abs(da) + Eda, np.abs(np.asarray(Wf, np.float64)), H, W)
    inh = dgrad7(Eda, np.abs(np.asarray(Wf, np.float64)), H, W)
    if f32:
        E["dx"] = br.dot_bound(dx, S, DX_TERMS, br.REF_EXTRA) + inh
    else:
        E["dx"] = U24 * np.abs(dx) + DX_TERMS * U53 * S + inh
    R["dx"] = dx
    return R, E


def unfolded(p, x, a, gp, Kc=None, f32=False):
    """(R, E) keyed "dx", "conv1.weight", "bn1.weight", "bn1.bias": backward() with the folded form of the raw
    parameters, then block_restatement.bn_unfold with the bounds carried through: what autograd leaves at x and at the
    stem's three parameters."""
    Wf, _ = fold(p)
    Rf, Ef = backward(x, a, gp, Wf, Kc=Kc, f32=f32)
    npix = int(np.prod(np.shape(a)[:3]))
    rs, es = br.bn_unfold(p["conv1"], p["bn1"], Rf["dW"], Rf["db"], Ef["dW"], Ef["db"], f32=f32, SdW=Ef["S:dW"],
                          Sdb=Ef["S:db"], npix=npix)
    R, E = {"dx": Rf["dx"]}, {"dx": Ef["dx"]}
    for k, r, e in zip(("conv1.weight", "bn1.weight", "bn1.bias"), rs, es):
        R[k], E[k] = r, e
    return R, E


ratio = br.ratio


def margins(p, x):
    """The smallest of |pre-activation| and, over the pooling windows with a positive maximum, the lead of the largest
    cell over the second largest: a forward deviating by less than this takes the same branches."""
    Wf, bf = fold(p)
    z = conv7(x, Wf) + np.asarray(bf, np.float64)
    a = np.maximum(z, 0.0)
    B, oh, ow, C = a.shape
    ph, pw = -(-oh // 2), -(-ow // 2)
    ap = np.full((B, 2 * ph + 1, 2 * pw + 1, C), -np.inf)
    ap[:, 1:oh + 1, 1:ow + 1] = a
    cells = np.stack([ap[:, dy:dy + 2 * ph:2, dx:dx + 2 * pw:2] for dy in range(3) for dx in range(3)], -1)
    top = np.sort(cells, -1)[..., -2:]
    gap = np.where(top[..., 1] > 0, top[..., 1] - top[..., 0], 1.0)
    return float(min(np.abs(z).min(), gap.min()))


def condition_image(p, x, margin=MARGIN, steps=4000, rate=2e-4):
    """chain_restatement.condition_image's idea at the stem's size: ``x`` moved by gradient descent on
    sum max(0, 2 margin - |v|) over the pre-activations and the window leads until margins() of its float32 rounding is
    at least ``margin``."""
    import torch
    import torch.nn.functional as F
    Wf, bf = (torch.from_numpy(np.asarray(v, np.float64)) for v in fold(p))
    x = np.asarray(x, np.float64)
    for it in range(steps):
        x32 = x.astype(np.float32)
        if it % 5 == 0 and margins(p, x32) >= margin:
            return x32
        with torch.enable_grad():  # whatever the process-wide switch is at
            t = torch.from_numpy(x).requires_grad_()
            z = F.conv2d(t, Wf, bf, 2, 3)
            act = F.relu(z)
            B, C, oh, ow = act.shape
            top = F.unfold(act, 3, 1, 1, 2).reshape(B, C, 9, -1).topk(2, 2).values
            gap = torch.where(top[:, :, 0] > 0, top[:, :, 0] - top[:, :, 1], torch.ones_like(top[:, :, 0]))
            (F.relu(2 * margin - z.abs()).sum() + F.relu(2 * margin - gap).sum()).backward()
        x = x - rate * min(6.0, 1.0 + it / 40.0) * t.grad.numpy()
    raise RuntimeError(f"condition_image: margin {margins(p, x.astype(np.float32)):.3g} after {steps} steps")


def draw_case(B, H, W, seed):
    """Seeded maps of one shape, float32: x, gp (about half exact zeros) and the ``a`` of a gradient-only case
    (non-negative, about half exact zeros, a few exact ties between neighbours)."""
    rng = np.random.default_rng(seed)
    oh, ow, ph, pw = sizes(H, W)
    a = br._half_zero(rng, (B, oh, ow, 64), True)
    if ow > 1:
        tie = rng.random((B, oh, ow - 1, 64)) < 0.1
        a[:, :, 1:] = np.where(tie, a[:, :, :-1], a[:, :, 1:])
    return dict(x=rng.standard_normal((B, 3, H, W)).astype(np.float32), gp=br._half_zero(rng, (B, ph, pw, 64)), a=a)
