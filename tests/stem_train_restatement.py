"""The stem of fpn_resnet_18 (models/fpn_resnet.py:179-182: conv1 7x7 / 2 / pad 3 without bias, bn1, ReLU,
MaxPool2d(3, 2, 1)) in train() mode, bn1 with batch statistics, and its gradients restated in numpy float64, with the
error bounds the GPU kernels (csrc/stem_train_kernel.h and the kernels it reuses) are held to.  conv7, patches, the
pool adjoint and dgrad7 are tests/stem_restatement.py's; the statistics, coef / apply, bn_backward and the running
update are tests/block_train_restatement.py's.  Neither is edited.

x is (B, 3, H, W) NCHW; z, a (B, oh, ow, 64) and p, gp (B, ph, pw, 64) are NHWC, oh = ceil(H / 2), ph = ceil(oh / 2),
n = B oh ow.  The parameters are the raw float32 conv1.weight (64, 3, 7, 7) and bn1 = (gamma, beta, running_mean,
running_var).

    z = conv7x7_2(x; W)        mean, var = batch mean / BIASED variance per channel
    a = ReLU(s z + t)          s = gamma / sqrt(var + eps), t = beta - mean s         p = maxpool3x3_2(a)
    dY = a > 0 ? (pool adjoint of gp by first maximum) : 0
    dbeta = sum dY   dgamma = invstd sum dY (z - mean)
    dZ = gamma invstd (dY - sum dY / n - (z - mean) invstd^2 sum dY (z - mean) / n)
    dW = wgrad_2(dZ, x)        dx = dgrad_2(dZ; W)

Bounds (u = 2^-24; r the float64 value; S the same expression on absolute values):
  z      float32 MFMA over the 147 entries inside one workgroup (the 13 padded entries are exact zeros):
         (147 + 1) u S + u |r| + 147 2^-126 (br.dot_bound).
  stats, apply, sums, dbeta, dgamma, dZ    block_train_restatement's forms, from the device's own z and float32
         statistics.  dY enters with E_dY = 3 u sum|gp won| (at most four float32 terms added, stem_restatement).
  dW     br._wgrad with K_c: (K_c + 1) u S + u |r| + chunks 2^-53 S + npix 2^-126 + the inherited E_dZ^T |patches|.
  dx     float64 accumulation of exact float32 products, at most 16 taps x 64 channels terms, rounded once:
         u |r| + 1024 2^-53 S + dgrad(E_dZ; |W|).
  pool   the maximum moves by at most the largest bound in its window.
``f32=True`` gives the reference's bounds (torch on the CPU in float32) as the two imported modules derive them.

A ratio error / bound above 1 means the kernel or this derivation is wrong; the bound is not to be widened.
"""
import numpy as np

import block_restatement as br
import block_train_restatement as tr
import stem_restatement as sr

U24, U53, TINY, EPS = br.U24, br.U53, br.TINY, br.EPS
REF_EXTRA = br.REF_EXTRA
MARGIN = 1e-3
MOMENTUM = tr.MOMENTUM
K = 147
GRADS = ("dx", "conv1.weight", "bn1.weight", "bn1.bias")
ratio = br.ratio
sizes = sr.sizes


def draw_params(seed):
    """stem_restatement.draw_params with the running statistics moved far from any batch's (means beyond +-2,
    variances in 4 .. 9), as block_train_restatement.draw_params moves them."""
    p = sr.draw_params(seed)
    rng = np.random.default_rng(seed + 77)
    g, b, _, _ = p["bn1"]
    p["bn1"] = (g, b, (np.where(rng.random(64) < 0.5, -1.0, 1.0) * rng.uniform(2.0, 3.0, 64)).astype(np.float32),
                rng.uniform(4.0, 9.0, 64).astype(np.float32))
    return p


def conv_stage(x, W, extra=0):
    """z = conv7x7_2(x; W) and its local bound."""
    r = sr.conv7(x, W)
    S = sr.conv7(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(W, np.float64)))
    return r, br.dot_bound(r, S, K, extra)


def pool(a):
    return sr.pool_argmax(a)[0]


def pool_bound(E):
    """The bound of a pooled map from the bound E of the map pooled: the largest in each window."""
    return sr.pool_argmax(E)[0]


def forward_chain(x, p, eps=EPS, f32=False, running=False):
    """The whole forward in float64 from x and the raw float32 parameters, every stage's bound carried to the end (the
    form of block_train_restatement.forward_chain's BatchNorm): (V, E) over z, pre, a, pooled and stats (2, 64).
    ``running``: a mutant for the host test, the eval() forward on the running statistics."""
    extra = REF_EXTRA if f32 else 0
    uu = U24 if f32 else U53
    V, E = {}, {}
    V["z"], E["z"] = conv_stage(x, p["conv1"], extra)
    g, b = (np.asarray(v, np.float64) for v in p["bn1"][:2])
    z2, E2 = tr._flat(V["z"]), tr._flat(E["z"])
    n = z2.shape[0]
    mean, var = tr.batch_stats(z2)
    xc = np.abs(z2 - mean)
    Em = E2.mean(0) + (n + 2) * uu * (np.abs(z2) + E2).mean(0) + U24 * np.abs(mean) + TINY
    cancel = (n + 8) * (U24 * var if f32 else U53 * ((z2 * z2).mean(0) + mean * mean))
    Ev = 2 * (xc * (E2 + Em)).mean(0) + ((E2 + Em) ** 2).mean(0) + cancel + U24 * var + TINY
    V["stats"], E["stats"] = np.array([mean, var]), np.array([Em, Ev])
    if running:
        mean, var = (np.asarray(v, np.float64) for v in p["bn1"][2:])
    inv, Einv = tr._invstd_interval(var, Ev, eps)
    sc = g * inv
    Es = np.abs(g) * Einv + (U24 + 4 * uu) * np.abs(sc) + (4 * U24 * np.abs(sc) if f32 else 0.0)
    t = b - mean * sc
    Et = Em * np.abs(sc) + (np.abs(mean) + Em) * Es + U24 * np.abs(t) + 4 * uu * (np.abs(b) + np.abs(mean * sc)) + TINY
    z, Ez = V["z"], E["z"]
    V["pre"] = sc * z + t
    E["pre"] = np.abs(sc) * Ez + (np.abs(z) + Ez) * Es + Et + (1 + extra) * U24 * (np.abs(sc * z) + np.abs(t)) + TINY
    V["a"], E["a"] = np.maximum(V["pre"], 0.0), E["pre"]
    V["pooled"], E["pooled"] = pool(V["a"]), pool_bound(E["a"])
    return V, E


def backward(x, maps, gp, p, eps=EPS, Kc=None, f32=False, drop_xhat=False):
    """(R, E) over GRADS: the gradients from the maps {z, a} and the float32 statistics maps["stats"] (2, 64) given
    (the masks and window maxima are read from ``a``).  Kc: the largest split-K chunk of dW in conv pixels (None: all
    pixels in one float32 accumulation).  R also holds "_dY" and "_dZ"."""
    x = np.asarray(x, np.float64)
    z, a, st = (np.asarray(maps[k], np.float64) for k in ("z", "a", "stats"))
    W = np.asarray(p["conv1"], np.float64)
    H, Wd = x.shape[2:]
    dap, dabs = sr.pool_adjoint(a, gp)
    dY, EdY = np.where(a > 0, dap, 0.0), np.where(a > 0, 3 * U24 * dabs, 0.0)
    R, E = {}, {}
    (dZ, R["bn1.weight"], R["bn1.bias"]), (EdZ, E["bn1.weight"], E["bn1.bias"]) = tr.bn_backward(
        dY, EdY, z, st[0], st[1], p["bn1"][0], eps, f32, drop_xhat)
    r, e, _ = br._wgrad(dZ, EdZ, sr.patches(x), Kc, f32)
    R["conv1.weight"], E["conv1.weight"] = r.reshape(64, 3, 7, 7), e.reshape(64, 3, 7, 7)
    dx = sr.dgrad7(dZ, W, H, Wd)
    S = sr.dgrad7(np.abs(dZ) + EdZ, np.abs(W), H, Wd)
    inh = sr.dgrad7(EdZ, np.abs(W), H, Wd)
    if f32:
        E["dx"] = br.dot_bound(dx, S, sr.DX_TERMS, REF_EXTRA) + inh
    else:
        E["dx"] = U24 * np.abs(dx) + sr.DX_TERMS * U53 * S + inh
    R["dx"], R["_dY"], R["_dZ"] = dx, dY, dZ
    return R, E


def eval_backward(x, a, gp, p, f32=False):
    """A mutant for the host test: stem_restatement's eval() gradient (bn1 folded with the running statistics, then
    unfolded) on the same maps, keyed as GRADS."""
    return sr.unfolded(p, x, a, gp, f32=f32)


running_update, running_bound = tr.running_update, tr.running_bound


def pool_lead(a):
    """The smallest lead of a window's largest cell over its second largest, over the windows with a positive maximum."""
    a = np.asarray(a, np.float64)
    B, oh, ow, C = a.shape
    ph, pw = -(-oh // 2), -(-ow // 2)
    ap = np.full((B, 2 * ph + 1, 2 * pw + 1, C), -np.inf)
    ap[:, 1:oh + 1, 1:ow + 1] = a
    cells = np.stack([ap[:, dy:dy + 2 * ph:2, dx:dx + 2 * pw:2] for dy in range(3) for dx in range(3)], -1)
    top = np.sort(cells, -1)[..., -2:]
    return float(np.where(top[..., 1] > 0, top[..., 1] - top[..., 0], 1.0).min())


def premises(x, p, eps=EPS):
    """(smallest |pre-activation|, smallest pool lead, smallest var / mean z^2 over the channels, smallest distance of
    a running statistic from the batch's in units of the batch's std / var)."""
    V, _ = forward_chain(x, p, eps)
    mean, var = V["stats"]
    cond = float((var / (tr._flat(V["z"]) ** 2).mean(0)).min())
    far = min(float((np.abs(p["bn1"][2] - mean) / np.sqrt(var)).min()), float((np.abs(p["bn1"][3] - var) / var).min()))
    return float(np.abs(V["pre"]).min()), pool_lead(V["a"]), cond, far


def condition_image(p, x, margin=MARGIN, steps=6000, rate=2e-4, eps=EPS):
    """stem_restatement.condition_image's idea under batch statistics: ``x`` moved by gradient descent on
    sum max(0, 2 margin - |v|) over the pre-activations and the window leads (the statistics differentiated through)
    until the float32 rounding of x has both at least ``margin``."""
    import torch
    import torch.nn.functional as F
    W = torch.from_numpy(np.asarray(p["conv1"], np.float64))
    g, b = (torch.from_numpy(np.asarray(v, np.float64)) for v in p["bn1"][:2])
    x = np.asarray(x, np.float64)
    for it in range(steps):
        x32 = x.astype(np.float32)
        if it % 5 == 0:
            pre, lead, _, _ = premises(x32, p, eps)
            if min(pre, lead) >= margin:
                return x32
        with torch.enable_grad():
            t = torch.from_numpy(x).requires_grad_()
            z = F.batch_norm(F.conv2d(t, W, None, 2, 3), None, None, g, b, True, 0.0, eps)
            act = F.relu(z)
            B, C, oh, ow = act.shape
            top = F.unfold(act, 3, 1, 1, 2).reshape(B, C, 9, -1).topk(2, 2).values
            gap = torch.where(top[:, :, 0] > 0, top[:, :, 0] - top[:, :, 1], torch.ones_like(top[:, :, 0]))
            (F.relu(2 * margin - z.abs()).sum() + F.relu(2 * margin - gap).sum()).backward()
        x = x - rate * min(6.0, 1.0 + it / 40.0) * t.grad.numpy()
    raise RuntimeError(f"condition_image: premises {premises(x.astype(np.float32), p, eps)[:2]} after {steps} steps")


def draw_case(B, H, W, seed):
    """Seeded float32 x (B, 3, H, W) and gp (B, ph, pw, 64), about half of gp exact zeros."""
    rng = np.random.default_rng(seed)
    _, _, ph, pw = sizes(H, W)
    return rng.standard_normal((B, 3, H, W)).astype(np.float32), br._half_zero(rng, (B, ph, pw, 64))
