"""One BasicBlock (models/fpn_resnet.py:42-71) in train() mode, BatchNorm with batch statistics, and its gradients
restated in numpy float64, with the error bounds the GPU kernels (csrc/block_train_kernel.h, csrc/block_kernel.h) are
held to.  Shapes, patches, conv3 / dgrad3, dot_bound and the weight-gradient bound are tests/block_restatement.py's.

    z1 = conv3x3_s(x; W1)      mean, var = batch mean / BIASED variance per channel over n = B oh ow values
    mid = ReLU(s1 z1 + t1)     s = gamma / sqrt(var + eps), t = beta - mean s
    z2 = conv3x3_1(mid; W2)    zd = conv1x1_s(x; Wd)      y = ReLU(s2 z2 + t2 + (x | sd zd + td))
    dY = y > 0 ? gy : 0        per BatchNorm, invstd = 1 / sqrt(var + eps):
        dbeta = A = sum dY     dgamma = invstd Bq,  Bq = sum dY (z - mean)
        dZ = gamma invstd (dY - A / n - (z - mean) invstd^2 Bq / n)
    dW2 = wgrad_1(dZ2, mid)    dA = mid > 0 ? dgrad_1(dZ2; W2) : 0     dZ1 = BatchNorm 1's backward of dA
    dW1 = wgrad_s(dZ1, x)      dWd = wgrad1x1_s(dZd, x)    dx = dgrad_s(dZ1; W1) + (dY | dgrad1x1_s(dZd; Wd))

What the device does, and what is therefore restated:
  * The statistics are one pass of float64 sums: mean = S1 / n, var = max(S2 / n - mean^2, 0), S1 = sum z,
    S2 = sum z^2 (the square of a float32 is exact in float64), each rounded once to float32.  stats_stage() takes the
    well-conditioned two-pass value as the truth and puts the one-pass form's cancellation into the bound:
    (n + 8) 2^-53 (S2 / n + mean^2) against var.
  * s and t are float64 expressions OF THE ROUNDED float32 mean and var, rounded once; the gradient entry reads the
    same float32 statistics array.  So for the device the statistics are inputs like the maps are, every stage is
    checked from the device's own inputs, and nothing is inherited from them.  The inherited terms (the error of
    mean and invstd carried into s, t and dZ) appear where the statistics themselves differ: in forward_chain(), which
    carries every stage's bound to the end of the block, and in the float32-reference form of backward().
  * BatchNorm's forward is one float32 FMA per element and one addition for the skip; its backward is float64 per
    element rounded once, from float64 sums in block order.

Bounds (u = 2^-24; r the float64 value; S the same expression on absolute values; E a bound an operand carries):
  conv   (K + 1) u S + u |r| + K 2^-126 (br.dot_bound), K = 9 Cin or Cin; + the stage applied to E with |W|.
  stats  mean: u |mean| + (n + 2) 2^-53 mean|z|;  var: u var + (n + 8) 2^-53 (S2 / n + mean^2).
  apply  v = fma(s32, z, t32): u |v| + E_s |z| + E_t with E_s = (u + 4 2^-53) |s|, E_t = u |t| + 4 2^-53 (|beta| + |mean s|);
         the skip: the other branch's bound + u |r|.  ReLU is 1-Lipschitz.
  sums   A: (n + 2) 2^-53 sum|dY| + sum E_dY;  Bq: (n + 4) 2^-53 sum |dY| |z - mean| + sum E_dY |z - mean|.
  dbeta  u |A| + E_A.    dgamma  (u + 4 2^-53) |dgamma| + invstd E_B.
  dZ     u |dZ| + |s| (E_dY + E_A / n + |z - mean| invstd^2 E_B / n + 8 2^-53 S_inner).
  dW     br._wgrad: (K_c + 1) u S + u |r| + chunks 2^-53 S + npix 2^-126 + the inherited E_dZ^T |patches|.
``f32=True`` gives the bounds of the reference, torch on the CPU in float32: every sum of n terms in float32 in any
order (n u where the device has n 2^-53; K_c = npix), REF_EXTRA further roundings per term, and ITS OWN float32
statistics of the same z in place of the ones the restatement is given: |mean_ref - mean| <= (n + 2) u mean|z| and
|var_ref - var| <= (n + 8) u var + 2 E_mean mean|z - mean| + E_mean^2, carried into invstd by the exact interval
1 / sqrt(var -+ E_var + eps) and from there into dgamma and dZ.

A ratio error / bound above 1 means the kernel or this derivation is wrong; the bound is not to be widened.
"""
import numpy as np

import block_restatement as br
from block_restatement import EPS, REF_EXTRA, TINY, U24, U53, block_shape, ratio  # noqa: F401

MARGIN = 1e-3  # every pre-activation of a conditioned case is at least this far from the ReLU's kink
BNS = ("bn1", "bn2", "bnd")
CONVS = ("conv1", "conv2", "convd")
PARAMS = tuple(k for c, b in zip(CONVS, BNS) for k in (c + ".weight", b + ".weight", b + ".bias"))
MOMENTUM = 0.1


def draw_params(layer, block, seed):
    """br.draw_params with the running statistics moved far from any batch's: means beyond +-2, variances in 4 .. 9
    (a batch of these cases has |mean| below 1 and a variance near 1)."""
    p = br.draw_params(layer, block, seed)
    rng = np.random.default_rng(seed + 77)
    for bn in BNS:
        if bn in p:
            g, b, mu, var = p[bn]
            c = g.shape[0]
            p[bn] = (g, b, (np.where(rng.random(c) < 0.5, -1.0, 1.0) * rng.uniform(2.0, 3.0, c)).astype(np.float32),
                     rng.uniform(4.0, 9.0, c).astype(np.float32))
    return p


def fixture_param_entries(layer, block, p):
    """The block's parameters as fixture entries {params/L<layer>b<block>/<key>: float32 array}."""
    pre = f"params/L{layer}b{block}/"
    out = {}
    for c, b in zip(CONVS, BNS):
        if c in p:
            out[pre + c], out[pre + b] = np.asarray(p[c], np.float32), np.stack([np.asarray(a, np.float32) for a in p[b]])
    return out


def fixture_params(g, layer, block):
    """The parameters a fixture stores for the block, in draw_params' form."""
    pre = f"params/L{layer}b{block}/"
    p = {}
    for c, b in zip(CONVS, BNS):
        if pre + c in g:
            p[c], p[b] = g[pre + c], tuple(g[pre + b])
    return p


def param_list(p):
    """The parameters in the entries' order: W1, gamma1, beta1, W2, gamma2, beta2[, Wd, gammad, betad]."""
    return [a for c, b in zip(CONVS, BNS) if c in p for a in (p[c], p[b][0], p[b][1])]


def wmat(W):
    """torch's (Cout, C, k, k) -> (Cout, taps C) in (tap, c) order, float64."""
    W = np.asarray(W, np.float64)
    return W.transpose(0, 2, 3, 1).reshape(W.shape[0], -1)


def conv_stage(x, W, s):
    """z = conv(x; W) for a 3x3 or 1x1 W in torch's layout, and its local bound."""
    x = np.asarray(x, np.float64)
    Wm = wmat(W)
    if W.shape[2] == 3:
        r, S = br.conv3(x, Wm, s), br.conv3(np.abs(x), np.abs(Wm), s)
    else:
        r, S = x[:, ::s, ::s] @ Wm.T, np.abs(x)[:, ::s, ::s] @ np.abs(Wm).T
    return r, br.dot_bound(r, S, Wm.shape[1])


def _flat(z):
    return np.asarray(z, np.float64).reshape(-1, np.shape(z)[-1])


def batch_stats(z):
    """(mean, biased var) per channel in float64, two-pass."""
    z = _flat(z)
    mean = z.mean(0)
    return mean, ((z - mean) ** 2).mean(0)


def batch_stats_one_pass(z):
    """The device's formula: mean = S1 / n, var = max(S2 / n - mean^2, 0)."""
    z = _flat(z)
    n = z.shape[0]
    mean = z.sum(0) / n
    return mean, np.maximum((z * z).sum(0) / n - mean * mean, 0.0)


def stats_stage(z):
    """((mean, var), (E_mean, E_var)) of the map z the device itself wrote."""
    z2 = _flat(z)
    n = z2.shape[0]
    mean, var = batch_stats(z2)
    Em = U24 * np.abs(mean) + (n + 2) * U53 * np.abs(z2).mean(0) + TINY
    Ev = U24 * var + (n + 8) * U53 * ((z2 * z2).mean(0) + mean * mean) + TINY
    return (mean, var), (Em, Ev)


def coef(gamma, beta, mean, var, eps=EPS):
    """(s, t, E_s, E_t): float64 from the float32 operands, and the bounds of the device's float32 pair."""
    gamma, beta, mean, var = (np.asarray(v, np.float64) for v in (gamma, beta, mean, var))
    s = gamma / np.sqrt(var + eps)
    t = beta - mean * s
    return s, t, (U24 + 4 * U53) * np.abs(s), U24 * np.abs(t) + 4 * U53 * (np.abs(beta) + np.abs(mean * s)) + TINY


def apply_stage(z, c, x=None, zd=None, cd=None):
    """out = ReLU(s z + t [+ x | + sd zd + td]) from the maps and float32 statistics the device read; c, cd = coef()."""
    def one(z, c):
        s, t, Es, Et = c
        z = np.asarray(z, np.float64)
        v = s * z + t
        return v, U24 * np.abs(v) + Es * np.abs(z) + Et + TINY

    v, E = one(z, c)
    if zd is not None:
        v2, E2 = one(zd, cd)
        v, E = v + v2, E + E2 + U24 * np.abs(v + v2)
    elif x is not None:
        v = v + np.asarray(x, np.float64)
        E = E + U24 * np.abs(v)
    return np.maximum(v, 0.0), E, v


def _invstd_interval(var, Evar, eps):
    inv = 1.0 / np.sqrt(var + eps)
    hi = 1.0 / np.sqrt(np.maximum(var - Evar, 0.0) + eps)
    lo = 1.0 / np.sqrt(var + Evar + eps)
    return inv, np.maximum(hi - inv, inv - lo)


def ref_stats_error(z, mean):
    """(E_mean, E_var): how far float32 statistics of z formed in any order lie from the float64 ones."""
    z2 = _flat(z)
    n = z2.shape[0]
    xc = z2 - mean
    Em = (n + 2) * U24 * np.abs(z2).mean(0) + TINY
    return Em, (n + 8) * U24 * (xc * xc).mean(0) + 2 * Em * np.abs(xc).mean(0) + Em * Em + TINY


def bn_backward(dY, EdY, z, mean, var, gamma, eps=EPS, f32=False, drop_xhat=False):
    """((dZ, dgamma, dbeta), (E_dZ, E_dgamma, E_dbeta)) of one BatchNorm from the float32 statistics given.
    ``drop_xhat``: a mutant for the host test, dZ without its sum dY (z - mean) term."""
    shape = np.shape(dY)
    dY, EdY, z = _flat(dY), _flat(EdY), _flat(z)
    mean, var, gamma = (np.asarray(v, np.float64) for v in (mean, var, gamma))
    n = dY.shape[0]
    uu = U24 if f32 else U53
    nn = n + 2 + (REF_EXTRA if f32 else 0)
    Em, Ev = ref_stats_error(z, mean) if f32 else (0.0, 0.0)
    inv, Einv = _invstd_interval(var, Ev, eps)
    Einv = Einv + 4 * uu * inv
    Einv2 = 2 * inv * Einv + Einv * Einv
    xc = z - mean
    aY = np.abs(dY) + EdY
    A, Bq = dY.sum(0), (dY * xc).sum(0)
    SA, SB = aY.sum(0), (aY * (np.abs(xc) + Em)).sum(0)
    EA = nn * uu * SA + EdY.sum(0)
    EB = (nn + 2) * uu * SB + (EdY * np.abs(xc)).sum(0) + Em * SA
    dbeta, dgamma = A, inv * Bq
    Edbeta = U24 * np.abs(A) + EA
    Edgamma = (U24 + 4 * uu) * np.abs(dgamma) + inv * EB + Einv * (np.abs(Bq) + EB) + TINY
    s = gamma * inv
    Es = np.abs(gamma) * Einv + 2 * uu * np.abs(s)
    i2 = inv * inv
    inner = dY - A / n - (0.0 if drop_xhat else xc * i2 * Bq / n)
    Sinner = np.abs(dY) + np.abs(A) / n + np.abs(xc) * i2 * np.abs(Bq) / n
    Einner = (EdY + EA / n + ((np.abs(xc) + Em) * (i2 + Einv2) * EB + Em * i2 * np.abs(Bq) + np.abs(xc) * Einv2 * np.abs(Bq)) / n
              + (10 if f32 else 8) * uu * Sinner)
    dZ = s * inner
    EdZ = U24 * np.abs(dZ) + np.abs(s) * Einner + Es * (np.abs(inner) + Einner) + TINY
    return (dZ.reshape(shape), dgamma, dbeta), (EdZ.reshape(shape), Edgamma, Edbeta)


def backward(x, maps, gy, p, s, eps=EPS, Kc=None, f32=False, drop_xhat=False):
    """(R, E) over "dx" and PARAMS (the downsample's absent without one): the gradients from the maps {z1, mid, z2,
    zd, y}, the float32 statistics maps["stats"] (nbn, 2, Cout) and the raw parameters p, dW in torch's layouts.
    Kc: the largest split-K chunk in output pixels (None: all pixels in one float32 accumulation)."""
    x, gy = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    m = {k: np.asarray(v, np.float64) for k, v in maps.items() if v is not None}
    st = m["stats"]
    ds = "convd" in p
    W1, W2 = wmat(p["conv1"]), wmat(p["conv2"])
    B, h, w, cin = x.shape
    cout = W1.shape[0]
    oh, ow = gy.shape[1:3]
    extra = REF_EXTRA if f32 else 0
    R, E = {}, {}
    dY = np.where(m["y"] > 0, gy, 0.0)
    z0 = np.zeros_like(dY)
    (dZ2, R["bn2.weight"], R["bn2.bias"]), (EZ2, E["bn2.weight"], E["bn2.bias"]) = bn_backward(
        dY, z0, m["z2"], st[1, 0], st[1, 1], p["bn2"][0], eps, f32, drop_xhat)
    r, e, _ = br._wgrad(dZ2, EZ2, br.patches(m["mid"], 1), Kc, f32)
    R["conv2.weight"], E["conv2.weight"] = br._torch_w(r, cout, 9), br._torch_w(e, cout, 9)
    dap = br.dgrad3(dZ2, W2, 1, oh, ow)
    Eap = br.dot_bound(dap, br.dgrad3(np.abs(dZ2) + EZ2, np.abs(W2), 1, oh, ow), 9 * cout, extra) + \
        br.dgrad3(EZ2, np.abs(W2), 1, oh, ow)
    dA, EdA = np.where(m["mid"] > 0, dap, 0.0), np.where(m["mid"] > 0, Eap, 0.0)
    (dZ1, R["bn1.weight"], R["bn1.bias"]), (EZ1, E["bn1.weight"], E["bn1.bias"]) = bn_backward(
        dA, EdA, m["z1"], st[0, 0], st[0, 1], p["bn1"][0], eps, f32, drop_xhat)
    r, e, _ = br._wgrad(dZ1, EZ1, br.patches(x, s), Kc, f32)
    R["conv1.weight"], E["conv1.weight"] = br._torch_w(r, cout, 9), br._torch_w(e, cout, 9)
    dx = br.dgrad3(dZ1, W1, s, h, w)
    S = br.dgrad3(np.abs(dZ1) + EZ1, np.abs(W1), s, h, w)
    inh = br.dgrad3(EZ1, np.abs(W1), s, h, w)
    K = 9 * cout
    if not ds:
        dx, S = dx + dY, S + np.abs(dY)
    else:
        Wd = wmat(p["convd"])
        (dZd, R["bnd.weight"], R["bnd.bias"]), (EZd, E["bnd.weight"], E["bnd.bias"]) = bn_backward(
            dY, z0, m["zd"], st[2, 0], st[2, 1], p["bnd"][0], eps, f32, drop_xhat)
        sk, Ssk, isk = np.zeros_like(dx), np.zeros_like(dx), np.zeros_like(dx)
        sk[:, ::s, ::s] = dZd @ Wd
        Ssk[:, ::s, ::s] = (np.abs(dZd) + EZd) @ np.abs(Wd)
        isk[:, ::s, ::s] = EZd @ np.abs(Wd)
        dx, S, K, inh = dx + sk, S + Ssk, K + cout, inh + isk
        r, e, _ = br._wgrad(dZd, EZd, x[:, ::s, ::s][:, :, :, None, :], Kc, f32)
        R["convd.weight"], E["convd.weight"] = br._torch_w(r, cout, 1), br._torch_w(e, cout, 1)
    R["dx"], E["dx"] = dx, br.dot_bound(dx, S, K, extra) + inh
    R["_dZ"] = dict(bn1=dZ1, bn2=dZ2, **(dict(bnd=dZd) if ds else {}))
    R["_dY"] = dict(bn1=dA, bn2=dY, bnd=dY)
    return R, E


def forward_chain(x, p, s, eps=EPS, f32=False):
    """The whole forward in float64 from x and the raw float32 parameters, every stage's bound carried to the end:
    (V, E) over z1, mid, z2[, zd], y, pre1, pre2 (the pre-activations) and stats (nbn, 2, Cout).  ``f32``: the
    reference's form."""
    x = np.asarray(x, np.float64)
    extra = REF_EXTRA if f32 else 0
    uu = U24 if f32 else U53
    V, E = {}, {}

    def conv(src, Esrc, W, stride):
        Wm = wmat(W)
        if W.shape[2] == 3:
            f = lambda a, M: br.conv3(a, M, stride)  # noqa: E731
        else:
            f = lambda a, M: np.asarray(a)[:, ::stride, ::stride] @ M.T  # noqa: E731
        r = f(src, Wm)
        return r, br.dot_bound(r, f(np.abs(src) + Esrc, np.abs(Wm)), Wm.shape[1], extra) + f(Esrc, np.abs(Wm))

    def bn(z, Ez, bnp):
        g, b = (np.asarray(v, np.float64) for v in bnp[:2])
        z2, E2 = _flat(z), _flat(Ez)
        n = z2.shape[0]
        mean, var = batch_stats(z2)
        xc = np.abs(z2 - mean)
        Em = E2.mean(0) + (n + 2) * uu * (np.abs(z2) + E2).mean(0) + U24 * np.abs(mean) + TINY
        cancel = (n + 8) * (U24 * var if f32 else U53 * ((z2 * z2).mean(0) + mean * mean))
        Ev = 2 * (xc * (E2 + Em)).mean(0) + ((E2 + Em) ** 2).mean(0) + cancel + U24 * var + TINY
        inv, Einv = _invstd_interval(var, Ev, eps)
        sc = g * inv
        Es = np.abs(g) * Einv + (U24 + 4 * uu) * np.abs(sc) + (4 * U24 * np.abs(sc) if f32 else 0.0)
        t = b - mean * sc
        Et = Em * np.abs(sc) + (np.abs(mean) + Em) * Es + U24 * np.abs(t) + 4 * uu * (np.abs(b) + np.abs(mean * sc)) + TINY
        v = sc * z + t
        Ev_ = np.abs(sc) * Ez + (np.abs(z) + Ez) * Es + Et + (1 + extra) * U24 * (np.abs(sc * z) + np.abs(t)) + TINY
        return v, Ev_, (mean, var), (Em, Ev)

    V["z1"], E["z1"] = conv(x, np.zeros_like(x), p["conv1"], s)
    V["pre1"], E["pre1"], st1, Est1 = bn(V["z1"], E["z1"], p["bn1"])
    V["mid"], E["mid"] = np.maximum(V["pre1"], 0.0), E["pre1"]
    V["z2"], E["z2"] = conv(V["mid"], E["mid"], p["conv2"], 1)
    v2, Ev2, st2, Est2 = bn(V["z2"], E["z2"], p["bn2"])
    sts, Ests = [st1, st2], [Est1, Est2]
    if "convd" in p:
        V["zd"], E["zd"] = conv(x, np.zeros_like(x), p["convd"], s)
        vd, Evd, std, Estd = bn(V["zd"], E["zd"], p["bnd"])
        sts.append(std)
        Ests.append(Estd)
        V["pre2"] = v2 + vd
        E["pre2"] = Ev2 + Evd + U24 * np.abs(V["pre2"])
    else:
        V["pre2"] = v2 + x
        E["pre2"] = Ev2 + U24 * np.abs(V["pre2"])
    V["y"], E["y"] = np.maximum(V["pre2"], 0.0), E["pre2"]
    V["stats"], E["stats"] = np.array(sts), np.array(Ests)
    return V, E


def running_update(before, stat, n, which, momentum=MOMENTUM):
    """nn.BatchNorm2d's train() update of a running buffer: (1 - m) before + m stat, the variance unbiased by
    n / (n - 1).  ``which``: 0 mean, 1 var."""
    f = n / (n - 1.0) if which else 1.0
    return (1.0 - momentum) * np.asarray(before, np.float64) + momentum * f * np.asarray(stat, np.float64)


def running_bound(before, stat, Estat, n, which, momentum=MOMENTUM):
    """Bound of a float32 evaluation of running_update() from a statistic that carries Estat."""
    f = n / (n - 1.0) if which else 1.0
    mag = (1.0 - momentum) * np.abs(before) + momentum * f * (np.abs(stat) + Estat)
    return momentum * f * Estat + 4 * U24 * mag + TINY


def draw_x(layer, block, B, h, w, seed):
    cin, cout, s, _ = block_shape(layer, block)
    rng = np.random.default_rng(seed)
    osh = (B, -(-h // s), -(-w // s), cout)
    return rng.standard_normal((B, h, w, cin)).astype(np.float32), rng.standard_normal(osh).astype(np.float32)


def premises(x, p, s, eps=EPS):
    """(smallest |pre-activation|, largest pre-activation bound of either form, smallest var / mean z^2 over the
    BatchNorms' channels, smallest distance of a running statistic from the batch's in units of the batch's std / var)."""
    V, E = forward_chain(x, p, s, eps)
    _, E32 = forward_chain(x, p, s, eps, f32=True)
    margin = min(float(np.abs(V["pre1"]).min()), float(np.abs(V["pre2"]).min()))
    worst = max(float((E["pre1"] + E32["pre1"]).max()), float((E["pre2"] + E32["pre2"]).max()))
    cond, far = np.inf, np.inf
    for i, (bn, zk) in enumerate(zip(BNS, ("z1", "z2", "zd"))):
        if bn not in p:
            continue
        mean, var = V["stats"][i]
        cond = min(cond, float((var / (_flat(V[zk]) ** 2).mean(0)).min()))
        far = min(far, float((np.abs(p[bn][2] - mean) / np.sqrt(var)).min()), float((np.abs(p[bn][3] - var) / var).min()))
    return margin, worst, cond, far
