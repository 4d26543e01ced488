"""CPU restatement of the scaled-fp16 convolution arithmetic (SFA_MATH_FP16X3 / SFA_MATH_FP16) — a
helper of tests/test_math_fp16_host.py, tests/test_gpu_math_fp16.py and tools/fp16_error_budget.py.

What the library specifies (include/sfa_hip.h sfa_math, csrc/conv.h, csrc/model.hip, csrc/pack_row.h), restated in torch:

* BatchNorm (eps 1e-5) folded as sfa_pack_weights does: scale = g / sqrt(var + eps) and
  shift = b - mean * scale in f64, W = f32(w * scale); a block's conv2 and its 1x1 downsample are one
  conv over two K-segments with bias f32(shift2 + shift_ds).
* Weight scale per output channel n (pack_row.h pack_row_scale): e[n] = floor(log2 max_k |W[n][k]|) over the
  whole K-concatenated row, W * 2^(13 - e[n]); zero rows keep scale 1.
* Activation scale per tensor and frame (conv.h amax_frame_scale): 2^(13 - e) for max |x| in [2^e, 2^(e+1))
  over the conv's input segments; zero -> 1.
* terms = 1 (SFA_MATH_FP16): each scaled operand rounded once to fp16 (round-to-nearest-even), one product.
  terms = 2 (SFA_MATH_FP16X3): scaled operand = hi + lo with hi = fp16(.), lo = fp16(. - hi), products
  hi*hi + hi*lo + lo*hi.
* Accumulation in f64 (the kernels accumulate in f32: their summation order is not part of the arithmetic),
  scaled back by the two powers of two, + bias (+ residual), ReLU; every tensor the library keeps in device
  memory is rounded to f32.
* The stem and the FPN 1x1 convs always use terms = 2 (model.hip); the FPN convs in the commuted form the
  library runs: up(W_a x) + W_b skip + b, W_a x at the low resolution stored as f32.  (The patch stem scales
  every 16 x 16 tile by its own maximum; here the frame's: both are fp16x3-exact to ~1e-7.)
* Heads: conv3x3 (terms) -> + bias -> ReLU -> 1x1 conv in full precision, level 0 nearest-resized, KFPN
  softmax-weighted sum.
"""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def _pow2_scale(mx):
    """2^(13 - floor(log2 mx)) per element of mx (f32 maxima); 1 where mx == 0."""
    mx = mx.to(torch.float32)
    _, e = torch.frexp(mx)  # mx = m 2^e, m in [0.5, 1): floor(log2 mx) = e - 1
    e = torch.clamp(e - 1, -100, 100)
    s = torch.ldexp(torch.ones_like(mx), 13 - e)
    return torch.where(mx > 0, s, torch.ones_like(mx)).to(F64)


def round_terms(v, terms):
    """v (f64 holding f32 values, already scaled) -> (hi, lo) as f64; lo is None for terms = 1."""
    v32 = v.to(torch.float32)
    hi = v32.to(torch.float16)
    if terms == 1:
        return hi.to(F64), None
    lo = (v32 - hi.to(torch.float32)).to(torch.float16)
    return hi.to(F64), lo.to(F64)


def fold_bn(sd, conv, bn):
    """f32 OIHW weight with BN folded, f64 shift — as pack_row.h pack_bn_fold and the gather of pack_host.h."""
    w = sd[conv + ".weight"].to(F64)
    scale = sd[bn + ".weight"].to(F64) / torch.sqrt(sd[bn + ".running_var"].to(F64) + 1e-5)
    shift = sd[bn + ".bias"].to(F64) - sd[bn + ".running_mean"].to(F64) * scale
    return (w * scale.view(-1, 1, 1, 1)).to(torch.float32), shift


def qconv(segs, bias, terms, relu=False, res=None, wrow_max=None, act_max=None):
    """One implicit-GEMM conv over K-segments [(x, w, stride, pad)]: x (B, C, H, W) f64 holding f32 values,
    w (O, I, KH, KW) f32.  wrow_max: the packed row's max |w| per output channel when the row is wider than
    these segments (a K-slice of a packed conv); act_max: per-frame max |x| (B,) when it is not the
    segments' own.  Returns f64 holding f32 values."""
    if wrow_max is None:
        wrow_max = torch.stack([w.abs().flatten(1).max(1).values for _, w, _, _ in segs]).max(0).values
    if act_max is None:
        act_max = torch.stack([x.abs().flatten(1).max(1).values for x, _, _, _ in segs]).max(0).values
    sw = _pow2_scale(wrow_max).view(-1, 1, 1, 1)
    sx = _pow2_scale(act_max).view(-1, 1, 1, 1)
    acc = None
    for x, w, stride, pad in segs:
        xh, xl = round_terms(x * sx, terms)
        wh, wl = round_terms(w.to(F64) * sw, terms)
        y = F.conv2d(xh, wh if terms == 1 else wh + wl, None, stride, pad)
        if terms == 2:
            y = y + F.conv2d(xl, wh, None, stride, pad)
        acc = y if acc is None else acc + y
    y = acc / sx / sw.view(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.to(F64).view(1, -1, 1, 1)
    if res is not None:
        y = y + res
    if relu:
        y = F.relu(y)
    return y.to(torch.float32).to(F64)


def head_level(sd, inp, level, heads, terms, act_max=None):
    """All heads of one FPN level: {head: (B, c, H, W) f64 (f32 values)} — conv3x3 at `terms`, the rest f32-class."""
    out = {}
    # the level's 3x3 convs are one packed conv (N = 64 * heads): each row has its own weight scale
    for head in heads:
        p = f"fpn{level}_{head}"
        h = qconv([(inp, sd[p + ".0.weight"], 1, 1)], sd[p + ".0.bias"], terms, relu=True, act_max=act_max)
        # (h stays in registers on the GPU: not rounded again; qconv's f32 rounding of it is below 1e-7)
        y = F.conv2d(h, sd[p + ".2.weight"].to(F64), sd[p + ".2.bias"].to(F64))
        out[head] = y.to(torch.float32).to(F64)
    return out


def _amax(x):
    return x.abs().flatten(1).max(1).values


def forward(sd, x, heads, terms, return_levels=False, head_terms=None):
    """sd: reference state_dict of torch CPU tensors; x (B, 3, H, W) f32.  Body convs and heads at `terms`
    (1 or 2), stem and FPN at 2; head_terms = 2 restates SFA_MATH_FP16 for a head count without a one-product
    heads kernel (anything but 5 heads: the heads then run fp16x3).  Returns {head: (B, c, H/4, W/4) f32 numpy}."""
    torch.set_grad_enabled(False)
    x = x.to(F64)
    w, sh = fold_bn(sd, "conv1", "bn1")
    y = qconv([(x, w, 2, 3)], sh, 2, relu=True)
    y = F.max_pool2d(y, 3, 2, 1)
    feats = []
    for li, stride in zip(range(1, 5), (1, 2, 2, 2)):
        for bi in range(2):
            p = f"layer{li}.{bi}"
            s = stride if bi == 0 else 1
            w1, sh1 = fold_bn(sd, p + ".conv1", p + ".bn1")
            t = qconv([(y, w1, s, 1)], sh1, terms, relu=True)
            w2, sh2 = fold_bn(sd, p + ".conv2", p + ".bn2")
            if p + ".downsample.0.weight" in sd:
                wd, shd = fold_bn(sd, p + ".downsample.0", p + ".downsample.1")
                y = qconv([(t, w2, 1, 1), (y, wd, s, 0)], (sh2 + shd).to(torch.float32), terms, relu=True)
            else:
                y = qconv([(t, w2, 1, 1)], sh2.to(torch.float32), terms, relu=True, res=y)
        feats.append(y)
    l1, l2, l3, l4 = feats

    def fpn(name, lo_in, skip):  # up(W_a lo_in) + W_b skip + b, both K-slices of one packed row
        wf = sd[name + ".weight"]
        ca = lo_in.shape[1]
        row_max = wf.abs().flatten(1).max(1).values
        lo = qconv([(lo_in, wf[:, :ca].contiguous(), 1, 0)], None, 2, wrow_max=row_max)
        up = F.interpolate(lo, scale_factor=2, mode="bilinear", align_corners=True).to(torch.float32).to(F64)
        return qconv([(skip, wf[:, ca:].contiguous(), 1, 0)], sd[name + ".bias"], 2, res=up, wrow_max=row_max)

    c1 = fpn("conv_up_level1", l4, l3)
    up2 = F.interpolate(c1, scale_factor=2, mode="bilinear", align_corners=True).to(torch.float32).to(F64)
    c2 = fpn("conv_up_level2", c1, l2)
    up3 = F.interpolate(c2, scale_factor=2, mode="bilinear", align_corners=True).to(torch.float32).to(F64)
    up4 = fpn("conv_up_level3", c2, l1)
    hm_h, hm_w = x.shape[2] // 4, x.shape[3] // 4
    # the heads' activation scale comes from the producing conv's recorded maximum (c1 / c2 / up4)
    lv = [head_level(sd, inp, f, heads, terms if head_terms is None else head_terms, act_max=_amax(src))
          for f, (inp, src) in enumerate(((up2, c1), (up3, c2), (up4, up4)))]
    ret = {}
    for head in heads:
        ls = [lv[f][head] for f in range(3)]
        ls = [F.interpolate(t, size=(hm_h, hm_w)) if t.shape[2] != hm_h or t.shape[3] != hm_w else t for t in ls]
        st = torch.stack(ls, dim=-1)
        ret[head] = (st * F.softmax(st, dim=-1)).sum(dim=-1).to(torch.float32).numpy()
    if return_levels:
        return ret, lv
    return ret


def rel_err(a, b):
    """max |a - b| / max(1, |b|) — the project's logit gate."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
