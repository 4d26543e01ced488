"""The whole training chain restated once more, independently of the per-operator restatements: stem, layer1..4, the
FPN neck, the fifteen heads, the KFPN combine and Compute_Loss as plain torch functional ops on the CPU, differentiated
by torch.autograd.  Nothing here calls a ``*_restatement.backward`` or anything under sfa/: the point is to share no
wiring with models/fpn_resnet.py (which level's gradient goes where, what is summed, which head comes first).

    stem     conv 7x7 / 2, BatchNorm (running statistics), ReLU, max-pool 3x3 / 2              -> pooled (B, 64, h, w)
    layerL   two BasicBlocks: ReLU(bn1(conv1 x)), ReLU(bn2(conv2 .) + (x | bn_d(conv_d x)))    -> out_layer1..4
    neck     z1 = conv_up_level1 cat(up l4, l3), u2 = up z1; z2 = conv_up_level2 cat(u2, l2), u3 = up z2;
             u4 = conv_up_level3 cat(u3, l1); up = bilinear x2, align_corners=True
    heads    per level f (inputs u2, u3, u4) and head: conv1x1(ReLU(conv3x3 + b)) + b; level 0 is at half resolution
             and brought to (h, w) by nearest-neighbour repetition
    combine  out = sum_f v_f softmax(v)_f
    loss     after tests/loss_restatement.py: clamped sigmoid of hm_cen and cen_offset, focal, L1, balanced L1 on the
             gathered slots; total = sum of the five

The heads are walked in the dict's insertion order, as the model's forward does (the modules were *registered* in
sorted() order, which only the state dict sees).

forward_backward() takes the input at one of three cuts: an image (B, 3, H, W), a pooled map (B, 64, h, w) or the four
backbone maps; ``perturb`` moves the output of every convolution stage, before its ReLU, by u GATE max(1, |v|) with u
uniform in [-1, 1] (the deviation the GPU forward is allowed per stage, tests/stage_cases.py GATE); ``mutant`` rewires
one thing the way a mistake in the model's Python would (tests/test_chain_host.py holds the gate against each).

Metric (metric()): per tensor m = ||got - ref|| / ||ref|| in float64, and the same per slice along the leading axis with
the denominator max(||ref_slice||, ||ref|| / sqrt(slices)), so that one wrong output channel of a 2.4 M element tensor
shows and a slice that happens to be near zero does not divide by nothing.  gate = 4 (noise32 + perturb), both
measured on the CPU by tests/golden/gen_chain_golden.py and stored in the fixture; never on the GPU.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import block_restatement as br
import loss_restatement as lr
import neck_restatement as nr

HEADS = {"hm_cen": 3, "cen_offset": 2, "direction": 2, "z_coor": 1, "dim": 3}  # the model's forward order
GATE = 1e-5  # stage_cases.GATE
EPS = 1e-5
GATE_FACTOR = 4.0
GATE_LIMIT = 1e-2
N_SAMPLES, N_PROJ, N_PERTURB = 256, 4, 8
MODEL_SEED = 2800
CASES = {
    "c2_64x96": dict(B=2, H=64, W=96, image_seed=11, label_seed=2),
    "c1_32x160": dict(B=1, H=32, W=160, image_seed=12, label_seed=4),
}
STEM = ("conv1.weight", "bn1.weight", "bn1.bias")
MUTANTS_RERUN = ("no_skip", "swap_levels", "avg_level0", "batch_stats", "transpose")
MUTANTS_POST = ("ds_bias", "sorted_heads", "twice")


# ------------------------------------------------------------------------------------------------ parameters, inputs
def draw_model(seed=MODEL_SEED):
    """The 186-entry state dict of fpn_resnet_18 as numpy arrays: the blocks from block_restatement.draw_params, the
    neck from neck_restatement.draw_params, the stem and the 60 head parameters drawn here.  Head biases are nonzero
    and no two are equal (a dropped bias, or another head's, cannot pass)."""
    rng = np.random.default_rng(seed)
    sd = {"conv1.weight": (rng.standard_normal((64, 3, 7, 7)) / np.sqrt(147.0)).astype(np.float32)}
    for k, v in zip(("weight", "bias", "running_mean", "running_var"),
                    (rng.uniform(0.5, 1.5, 64), 0.3 * rng.standard_normal(64), 0.3 * rng.standard_normal(64),
                     rng.uniform(0.5, 1.5, 64))):
        sd[f"bn1.{k}"] = v.astype(np.float32)
    for L in (1, 2, 3, 4):
        for b in (0, 1):
            sd.update(br.state_entries(L, b, br.draw_params(L, b, seed + 10 * L + b)))
    neck = nr.draw_params(seed + 1)
    for f in range(3):
        sd[f"conv_up_level{f + 1}.weight"] = neck[2 * f][:, :, None, None].copy()
        sd[f"conv_up_level{f + 1}.bias"] = neck[2 * f + 1]
    for f, cin in enumerate((256, 128, 64)):
        for head in sorted(HEADS):  # registration order of the modules
            c = HEADS[head]
            p = f"fpn{f}_{head}"
            sd[p + ".0.weight"] = (rng.standard_normal((64, cin, 3, 3)) / np.sqrt(9.0 * cin)).astype(np.float32)
            sd[p + ".0.bias"] = (rng.uniform(0.05, 0.3, 64) * rng.choice([-1.0, 1.0], 64)).astype(np.float32)
            sd[p + ".2.weight"] = (rng.standard_normal((c, 64, 1, 1)) / 8.0).astype(np.float32)
            sd[p + ".2.bias"] = (rng.uniform(0.05, 0.3, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
            if head == "hm_cen":  # the reference's initial heat-map bias: few cells start out as detections
                sd[p + ".2.bias"] = (sd[p + ".2.bias"] - np.float32(2.19)).astype(np.float32)
    biases = np.concatenate([v for k, v in sd.items() if k.startswith("fpn") and k.endswith(".bias")])
    assert np.all(biases != 0) and len(np.unique(biases)) == biases.size
    for k in [k for k in sd if k.endswith("running_var")]:
        sd[k[:-len("running_var")] + "num_batches_tracked"] = np.zeros((), np.int64)
    return sd


def parameter_names(sd):
    return [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def group_of(name):
    if name in STEM:
        return "stem"
    if name.startswith("layer") and "." in name:
        return "blocks"
    if name.startswith("conv_up_level"):
        return "neck"
    if name.startswith("fpn"):
        return "heads"
    return "inputs"  # x, pooled, layer1..4


def draw_inputs(case, image=None):
    """{image (B, 3, H, W) float32, labels, offsets, targets}: the targets are loss_restatement.build_targets_batch of
    synthetic.synthetic_labels on the (H / 4, W / 4) map, no flips.  The image is the seeded draw, or ``image``: the
    fixture's, which is that draw after condition_image()."""
    from sfa_hip import synthetic
    c = CASES[case]
    if image is None:
        rng = np.random.default_rng(c["image_seed"])
        image = rng.standard_normal((c["B"], 3, c["H"], c["W"])).astype(np.float32)
    assert image.shape == (c["B"], 3, c["H"], c["W"]) and image.dtype == np.float32
    labels, offsets = synthetic.synthetic_labels(c["B"], seed=c["label_seed"])
    tg, status = lr.build_targets_batch(labels, offsets, hm_size=(c["H"] // 4, c["W"] // 4))
    assert not status.any()
    return dict(image=image, labels=labels, offsets=offsets, targets=tg)


# ------------------------------------------------------------------------------------------------------- the forward
class _GradMap(torch.autograd.Function):
    """Identity whose backward passes the gradients through ``fn`` (the mutants)."""

    @staticmethod
    def forward(ctx, fn, *xs):
        ctx.fn = fn
        return tuple(x.view_as(x) for x in xs)

    @staticmethod
    def backward(ctx, *gs):
        return (None,) + tuple(ctx.fn(*gs))


class _Chain:
    def __init__(self, P, perturb, mutant):
        self.P, self.mutant = P, mutant
        self.rng = None if perturb is None else np.random.default_rng(perturb)
        self.pre = None  # a list: collects what goes into a ReLU or into the max-pool's choice (margins())

    def stage(self, v, relu=False):
        """The output of one convolution stage (``relu``: one that a ReLU follows)."""
        if relu and self.pre is not None:
            self.pre.append(v)
        if self.rng is None:
            return v
        u = torch.from_numpy(self.rng.uniform(-1.0, 1.0, tuple(v.shape))).to(v.dtype)
        return v + u * GATE * v.detach().abs().clamp(min=1.0)

    def bn(self, x, pre):
        P = self.P
        if self.mutant == "batch_stats":
            return F.batch_norm(x, None, None, P[pre + ".weight"], P[pre + ".bias"], True, 0.1, EPS)
        return F.batch_norm(x, P[pre + ".running_mean"], P[pre + ".running_var"], P[pre + ".weight"], P[pre + ".bias"],
                            False, 0.1, EPS)

    def stem(self, image):
        x = F.relu(self.stage(self.bn(F.conv2d(image, self.P["conv1.weight"], None, 2, 3), "bn1"), True))
        if self.pre is not None:  # the two largest of every pooling window (zero padding: x >= 0), where one is positive
            B, C, H, W = x.shape
            top = F.unfold(x, 3, 1, 1, 2).reshape(B, C, 9, -1).topk(2, 2).values
            gap = top[:, :, 0] - top[:, :, 1]
            self.pre.append(torch.where(top[:, :, 0] > 0, gap, torch.ones_like(gap)))
        return F.max_pool2d(x, 3, 2, 1)

    def block(self, x, L, b):
        P, pre = self.P, f"layer{L}.{b}"
        s = 2 if (b == 0 and L > 1) else 1
        a = F.relu(self.stage(self.bn(F.conv2d(x, P[pre + ".conv1.weight"], None, s, 1), pre + ".bn1"), True))
        z = self.bn(F.conv2d(a, P[pre + ".conv2.weight"], None, 1, 1), pre + ".bn2")
        skip = x
        if pre + ".downsample.0.weight" in P:
            skip = self.bn(F.conv2d(x, P[pre + ".downsample.0.weight"], None, s, 0), pre + ".downsample.1")
        return F.relu(self.stage(z + skip, True))

    def layers(self, pooled):
        outs, x = [], pooled
        for L in (1, 2, 3, 4):
            x = self.block(self.block(x, L, 0), L, 1)
            outs.append(x)
        return outs

    def neck(self, l1, l2, l3, l4):
        P = self.P
        if self.mutant == "no_skip":
            l1, l2, l3 = l1.detach(), l2.detach(), l3.detach()
        up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)  # noqa: E731
        z1 = self.stage(F.conv2d(torch.cat((up(l4), l3), 1), P["conv_up_level1.weight"], P["conv_up_level1.bias"]))
        u2 = up(z1)
        z2 = self.stage(F.conv2d(torch.cat((u2, l2), 1), P["conv_up_level2.weight"], P["conv_up_level2.bias"]))
        u3 = up(z2)
        u4 = self.stage(F.conv2d(torch.cat((u3, l1), 1), P["conv_up_level3.weight"], P["conv_up_level3.bias"]))
        return u2, u3, u4

    def detect(self, u2, u3, u4):
        P = self.P
        hm_h, hm_w = u4.shape[2:]
        if self.mutant == "transpose":  # the gradient of up_level3 read back with H and W exchanged
            (u3,) = _GradMap.apply(lambda g: (g.transpose(2, 3).contiguous().view(g.shape),), u3)
        ret = {}
        for head in HEADS:
            lv = []
            for f, x in enumerate((u2, u3, u4)):
                p = f"fpn{f}_{head}"
                hd = F.relu(self.stage(F.conv2d(x, P[p + ".0.weight"], P[p + ".0.bias"], 1, 1), True))
                lv.append(self.stage(F.conv2d(hd, P[p + ".2.weight"], P[p + ".2.bias"])))
            if self.mutant == "swap_levels":
                lv[1], lv[2] = _GradMap.apply(lambda g1, g2: (g2, g1), lv[1], lv[2])
            y0 = F.interpolate(lv[0], size=(hm_h, hm_w))  # nearest: every level-0 cell is read by 2 x 2 outputs
            if self.mutant == "avg_level0":
                y0 = y0.detach() + 0.25 * (y0 - y0.detach())
            v = torch.stack((y0, lv[1], lv[2]), -1)
            ret[head] = (v * F.softmax(v, -1)).sum(-1)
        return ret


def _gather(feat, ind):
    B, c = feat.shape[:2]
    return feat.reshape(B, c, -1).gather(2, ind[:, None, :].expand(B, c, ind.shape[1])).transpose(1, 2)  # (B, M, c)


def _balanced_l1(diff, alpha=0.5, gamma=1.5, beta=1.0):
    b = float(np.exp(gamma / alpha) - 1)
    small = alpha / b * (b * diff + 1) * torch.log(b * diff / beta + 1) - alpha * diff
    return torch.where(diff < beta, small, gamma * diff + gamma / b - alpha * beta)


def loss_terms(maps, tg, details=None):
    """The six losses in loss_restatement.LOSS_KEYS order as 0-dim tensors.  ``tg``: the targets as tensors (float
    ones in the maps' dtype).  ``details`` (a dict) receives what the premises look at."""
    p = torch.clamp(torch.sigmoid(maps["hm_cen"]), 1e-4, 1 - 1e-4)
    off = torch.clamp(torch.sigmoid(maps["cen_offset"]), 1e-4, 1 - 1e-4)
    gt = tg["hm_cen"]
    pos_m, neg_m = gt == 1, gt < 1
    pos = (torch.log(p) * (1 - p) ** 2)[pos_m].sum()
    neg = (torch.log(1 - p) * p ** 2 * (1 - gt) ** 4)[neg_m].sum()
    num_pos = int(pos_m.sum())
    hm = -neg if num_pos == 0 else -(pos + neg) / num_pos
    ind = tg["indices_center"]
    m = tg["obj_mask"].to(p.dtype)[:, :, None]
    msum = m.sum()
    out = {}
    for key, pred in (("cen_offset", off), ("direction", maps["direction"]), ("z_coor", maps["z_coor"]),
                      ("dim", maps["dim"])):
        a, b = _gather(pred, ind) * m, tg[key] * m
        d = (a - b).abs()
        out[key] = (d if key in ("cen_offset", "direction") else _balanced_l1(d)).sum() / (msum * pred.shape[1] + 1e-4)
        if details is not None:
            sel = m.expand_as(d) > 0
            details[f"diff/{key}"] = d[sel].detach().numpy().copy()
            if key == "cen_offset":
                details["gathered_sigmoid"] = a[sel].detach().numpy().copy()
    if details is not None:
        details["objects"] = tg["obj_mask"].sum(1).numpy().copy()
    total = hm + out["cen_offset"] + out["dim"] + out["direction"] + out["z_coor"]
    return [total, hm, out["cen_offset"], out["dim"], out["direction"], out["z_coor"]]


def _targets(tg, dtype):
    out = {}
    for k, v in tg.items():
        t = torch.from_numpy(np.ascontiguousarray(v))
        out[k] = t.to(torch.int64) if k in ("indices_center", "obj_mask") else t.to(dtype)
    return out


def forward_backward(state, inp, targets, dtype=torch.float64, perturb=None, mutant=None, inter=None, details=None):
    """(loss, maps, grads).  ``inp``: an image (B, 3, H, W), a pooled map (B, 64, h, w), or the four backbone maps
    (out_layer1..4) as a sequence; numpy, NCHW.  loss: the six terms (float64 array, LOSS_KEYS order); maps: the five
    outputs {head: (B, c, h, w)} as numpy in ``dtype``; grads: {parameter name: d total / d parameter} for every
    parameter behind the cut, plus "x" (the input; "layer1".."layer4" for the four maps) and, behind an image,
    "pooled".  ``perturb``: None or the seed of one draw of the per-stage deviation; ``mutant``: one of MUTANTS_RERUN;
    ``inter`` (a dict) receives the pooled map, out_layer1..4 and up_level2..4 as numpy."""
    P = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items() if not k.endswith("num_batches_tracked")}
    names = parameter_names(state)
    for k in names:
        P[k].requires_grad_()
    ch = _Chain(P, perturb, mutant)
    leaves, keep = {}, {}
    with torch.enable_grad():
        if isinstance(inp, (list, tuple)):
            ls = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_() for a in inp]
            leaves.update({f"layer{i + 1}": t for i, t in enumerate(ls)})
        else:
            x = torch.from_numpy(np.asarray(inp)).to(dtype).requires_grad_()
            leaves["x"] = x
            if x.shape[1] == 3:
                x = ch.stem(x)
                x.retain_grad()
                leaves["pooled"] = x
            keep["pooled"] = x
            ls = ch.layers(x)
        us = ch.neck(*ls)
        maps = ch.detect(*us)
        terms = loss_terms(maps, _targets(targets, dtype), details)
        terms[0].backward()
    if inter is not None:
        keep.update({f"layer{i + 1}": t for i, t in enumerate(ls)})
        keep.update({f"up_level{i + 2}": t for i, t in enumerate(us)})
        inter.update({k: t.detach().numpy().copy() for k, t in keep.items()})
    grads = {k: P[k].grad.numpy() for k in names if P[k].grad is not None}
    grads.update({k: t.grad.numpy() for k, t in leaves.items()})
    return (np.array([float(t.detach()) for t in terms]), {k: v.detach().numpy() for k, v in maps.items()}, grads)


MARGIN = 1e-3


def _pre_activations(state, image, grad=False):
    """(the image as a float64 tensor, every value a ReLU or the max-pool's choice depends on the sign of: the
    pre-activations of all ReLUs and, per pooling window with a positive maximum, the lead of the largest over the
    second)."""
    D = torch.float64
    P = {k: torch.from_numpy(np.asarray(v)).to(D) for k, v in state.items() if not k.endswith("num_batches_tracked")}
    ch = _Chain(P, None, None)
    ch.pre = []
    x = torch.from_numpy(np.asarray(image)).to(D).requires_grad_(grad)
    ch.detect(*ch.neck(*ch.layers(ch.stem(x))))
    return x, ch.pre


def margins(state, image):
    """The smallest |value| among _pre_activations(): a forward that deviates by less than this per element takes
    the same ReLU branches and pooling choices, so its gradient differs from the exact one continuously."""
    with torch.no_grad():
        return min(float(v.abs().min()) for v in _pre_activations(state, image)[1])


def condition_image(state, image, margin=MARGIN, steps=2000, rate=2e-4):
    """``image`` moved, by plain gradient descent on sum max(0, 2 margin - |v|) over _pre_activations(), until
    margins() of its float32 rounding is at least ``margin``.  A ReLU network's gradient jumps where a
    pre-activation changes sign: on a raw draw some of the 10^6 pre-activations lie within the forward's legitimate
    deviation of zero, and then two correct forwards disagree on a gradient by percents.  The generator runs this
    once and stores the image; the tests assert the margin on what is stored."""
    x = np.asarray(image, np.float64)
    for it in range(steps):
        x32 = x.astype(np.float32)
        if it % 5 == 0 and margins(state, x32) >= margin:
            return x32
        with torch.enable_grad():
            t, pre = _pre_activations(state, x, grad=True)
            sum(F.relu(2 * margin - v.abs()).sum() for v in pre).backward()
        x = x - rate * min(6.0, 1.0 + it / 40.0) * t.grad.numpy()  # the last few violators have small gradients
    raise RuntimeError(f"condition_image: margin {margins(state, x.astype(np.float32)):.3g} after {steps} steps")


def mutate_grads(grads, kind):
    """The mutants that are a rewiring of finished gradients (MUTANTS_POST); returns a new dict."""
    g = dict(grads)
    if kind == "ds_bias":  # the downsample's BatchNorm bias from conv1's db' instead of conv2's
        for L in (2, 3, 4):
            g[f"layer{L}.0.downsample.1.bias"] = grads[f"layer{L}.0.bn1.bias"]
    elif kind == "sorted_heads":  # the flat list of head gradients built in sorted() order, handed out in forward order
        for f in range(3):
            for mine, other in zip(HEADS, sorted(HEADS)):
                for leaf in (".0.weight", ".0.bias", ".2.weight", ".2.bias"):
                    a, b = f"fpn{f}_{mine}{leaf}", f"fpn{f}_{other}{leaf}"
                    if grads[a].shape == grads[b].shape:
                        g[a] = grads[b]
    elif kind == "twice":
        g["layer3.1.conv2.weight"] = 2 * grads["layer3.1.conv2.weight"]
    else:
        raise ValueError(kind)
    return g


# ------------------------------------------------------------------------------------------- metric, samples, gates
def metric(got, ref):
    """(m of the tensor, largest m of a slice along the leading axis), float64."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    n = ref.shape[0] if ref.ndim else 1
    d, r = (got - ref).reshape(n, -1), ref.reshape(n, -1)
    norm = float(np.sqrt((r * r).sum()))
    den = max(norm, 1e-300)
    rows = np.sqrt((d * d).sum(1)) / np.maximum(np.sqrt((r * r).sum(1)), den / np.sqrt(n))
    return np.array([float(np.sqrt((d * d).sum())) / den, float(rows.max())])


def _name_rng(name, what):
    return np.random.default_rng([zlib.crc32(name.encode()), what])


def sample_indices(name, size):
    """The N_SAMPLES seeded flat indices summary() reads (with repetitions where the tensor is small)."""
    return _name_rng(name, 1).integers(0, size, N_SAMPLES)


def summary(name, t):
    """(float32 norm, N_SAMPLES values at seeded flat indices, N_PROJ seeded +-1 projections in float64)."""
    flat = np.asarray(t).reshape(-1)
    idx = sample_indices(name, flat.size)
    rng = _name_rng(name, 2)
    f64 = flat.astype(np.float64)
    proj = np.array([float(np.dot(f64, rng.integers(0, 2, flat.size) * 2.0 - 1.0)) for _ in range(N_PROJ)])
    return np.float32(np.sqrt((f64 * f64).sum())), flat[idx].astype(np.float32), proj


def gates(g, case):
    """{tensor: (gate of the tensor form, gate of the slice form)} from the fixture's noise32 and perturb."""
    pre = f"{case}/noise32/"
    return {k[len(pre):]: GATE_FACTOR * (g[k] + g[f"{case}/perturb/{k[len(pre):]}"]) for k in g.files if k.startswith(pre)}


def worst_ratios(got, ref, gate, names):
    """{group: (largest m / gate over both forms, the tensor it is at)} over ``names``."""
    out = {}
    for k in names:
        q = float(np.max(metric(got[k], ref[k]) / gate[k]))
        grp = group_of(k)
        if grp not in out or q > out[grp][0]:
            out[grp] = (q, k)
    return out
