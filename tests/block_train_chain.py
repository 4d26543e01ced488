"""layer1..4 under train() as one chain: the eight BasicBlocks (models/fpn_resnet.py:184-187) on a pooled map, every
BatchNorm on batch statistics, restated in torch ops (F.conv2d, F.batch_norm(training=True)) and differentiated by
autograd, built as tests/chain_restatement.py builds its chain.  The loss is L = sum_L <g_L, out_layer_L> with seeded
cotangents g_L, so every output carries weight and every one of the 57 parameters and x gets a gradient.

The composed gate is §28's: gate(t) = GATE_FACTOR (noise32(t) + perturb(t)) in both forms of chain_restatement.metric,
where noise32 is the float32 CPU run of this very chain against the float64 one and perturb the float64 chain with
every stage (each convolution's and each BatchNorm's output) moved by GATE max(1, |v|) U(-1, 1), the per-stage
deviation the device's stages are held to.  tests/golden/gen_block_train_chain_golden.py measures both on the CPU
and stores them with the conditioned input: every pre-activation at least MARGIN from zero, so that a forward inside
its deviation takes the same ReLU branches.  The running buffers after the step are tensors of the chain like any
other and get a gate the same way."""
import numpy as np
import torch
import torch.nn.functional as F

import block_restatement as br
import block_train_restatement as tr
from chain_restatement import GATE, GATE_FACTOR, GATE_LIMIT, MARGIN, metric  # noqa: F401

SHAPE = (2, 64, 16, 24)
PARAM_SEED = 700  # block (L, b) draws tr.draw_params(L, b, PARAM_SEED + 10 L + b)
BLOCKS = [(L, b) for L in (1, 2, 3, 4) for b in (0, 1)]
LAYERS = ("out_layer1", "out_layer2", "out_layer3", "out_layer4")
MUTANTS = ("running_stats", "no_skip_grad", "bn_no_xhat")


def draw_state():
    """{state-dict name: float32 array} of the eight blocks: weights, BatchNorm weights, biases and running buffers."""
    sd = {}
    for L, b in BLOCKS:
        sd.update(br.state_entries(L, b, tr.draw_params(L, b, PARAM_SEED + 10 * L + b)))
    return sd


def parameter_names(sd):
    return [k for k in sd if not k.endswith(("running_mean", "running_var"))]


def cotangents():
    rng = np.random.default_rng(4100)
    B, _, h, w = SHAPE
    return [rng.standard_normal((B, 64 << i, h >> i, w >> i)).astype(np.float32) for i in range(4)]


class _DropXhat(torch.autograd.Function):
    """BatchNorm's normalisation whose backward forgets the sum dY x^ term (a mutant)."""

    @staticmethod
    def forward(ctx, z, eps):
        mean = z.mean((0, 2, 3), keepdim=True)
        inv = (z.var((0, 2, 3), unbiased=False, keepdim=True) + eps).rsqrt()
        ctx.inv = inv
        return (z - mean) * inv

    @staticmethod
    def backward(ctx, g):
        return ctx.inv * (g - g.mean((0, 2, 3), keepdim=True)), None


def forward_backward(state, x, dtype=torch.float64, perturb=None, mutant=None, want_pre=False):
    """(outs, grads, running, pre): the four maps, the gradients of L at "x" and the 57 parameters, the running buffers
    after the step {name: array}, and (``want_pre``) the smallest |pre-activation|.  ``perturb``: a numpy Generator
    that moves every stage's output by GATE max(1, |v|) U(-1, 1).  ``mutant``: one of MUTANTS."""
    P = {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in state.items()}  # copies: the buffers move in place
    for k in parameter_names(state):
        P[k].requires_grad_(True)
    xt = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    pre_min = [np.inf]

    def stage(v):
        if perturb is None:
            return v
        noise = torch.from_numpy(perturb.uniform(-1.0, 1.0, tuple(v.shape))).to(dtype)
        return v + GATE * torch.clamp(v.detach().abs(), min=1.0) * noise

    def bn(v, pre):
        rm, rv = P[pre + ".running_mean"], P[pre + ".running_var"]
        if mutant == "running_stats":
            return stage(F.batch_norm(v, rm, rv, P[pre + ".weight"], P[pre + ".bias"], False, tr.MOMENTUM, tr.EPS))
        if mutant == "bn_no_xhat":
            F.batch_norm(v.detach(), rm, rv, None, None, True, tr.MOMENTUM, tr.EPS)  # moves the buffers
            return stage(_DropXhat.apply(v, tr.EPS) * P[pre + ".weight"].view(1, -1, 1, 1) + P[pre + ".bias"].view(1, -1, 1, 1))
        return stage(F.batch_norm(v, rm, rv, P[pre + ".weight"], P[pre + ".bias"], True, tr.MOMENTUM, tr.EPS))

    def relu(v):
        if want_pre:
            pre_min[0] = min(pre_min[0], float(v.detach().abs().min()))
        return F.relu(v)

    outs, t = [], xt
    for L, b in BLOCKS:
        pre = f"layer{L}.{b}"
        ds = pre + ".downsample.0.weight" in P
        s = 2 if ds else 1
        mid = relu(bn(stage(F.conv2d(t, P[pre + ".conv1.weight"], stride=s, padding=1)), pre + ".bn1"))
        z = bn(stage(F.conv2d(mid, P[pre + ".conv2.weight"], padding=1)), pre + ".bn2")
        if ds:
            skip = bn(stage(F.conv2d(t, P[pre + ".downsample.0.weight"], stride=s)), pre + ".downsample.1")
        else:
            skip = t.detach() if mutant == "no_skip_grad" else t
        t = relu(z + skip)
        if b == 1:
            outs.append(t)
    sum((o * torch.from_numpy(g).to(dtype)).sum() for o, g in zip(outs, cotangents())).backward()
    grads = {k: P[k].grad.numpy() for k in parameter_names(state)}
    grads["x"] = xt.grad.numpy()
    running = {k: P[k].detach().numpy() for k in state if k.endswith(("running_mean", "running_var"))}
    return {n: o.detach().numpy() for n, o in zip(LAYERS, outs)}, grads, running, pre_min[0]


def tensors(outs, grads, running):
    """One flat dict over everything that is gated: out_layer*, grad/<name>, the running buffers."""
    d = dict(outs)
    d.update({"grad/" + k: v for k, v in grads.items()})
    d.update(running)
    return d


def condition_input(state, x, margin=MARGIN, steps=3000, rate=2e-4):
    """x moved by gradient descent on sum max(0, 2 margin - |pre-activation|) until the float32 rounding of it has
    every pre-activation at least ``margin`` from zero (chain_restatement.condition_image's scheme)."""
    D = torch.float64
    P = {k: torch.from_numpy(np.asarray(v)).to(D) for k, v in state.items()}
    x = np.asarray(x, np.float64)
    for it in range(steps):
        x32 = x.astype(np.float32)
        if it % 5 == 0 and forward_backward(state, x32, want_pre=True)[3] >= margin:
            return x32
        xt = torch.from_numpy(x).requires_grad_(True)
        pres, t = [], xt
        for L, b in BLOCKS:
            pre = f"layer{L}.{b}"
            ds = pre + ".downsample.0.weight" in P
            s = 2 if ds else 1
            bn = lambda v, k: F.batch_norm(v, None, None, P[k + ".weight"], P[k + ".bias"], True, 0.0, tr.EPS)  # noqa: E731
            p1 = bn(F.conv2d(t, P[pre + ".conv1.weight"], stride=s, padding=1), pre + ".bn1")
            z = bn(F.conv2d(F.relu(p1), P[pre + ".conv2.weight"], padding=1), pre + ".bn2")
            p2 = z + (bn(F.conv2d(t, P[pre + ".downsample.0.weight"], stride=s), pre + ".downsample.1") if ds else t)
            pres += [p1, p2]
            t = F.relu(p2)
        sum(F.relu(2 * margin - v.abs()).sum() for v in pres).backward()
        x = x - rate * min(6.0, 1.0 + it / 40.0) * xt.grad.numpy()
    raise RuntimeError("condition_input: the margin was not reached")


def gates(g):
    """{tensor: (gate of the tensor form, gate of the slice form)} from the fixture's noise32 and perturb."""
    return {k[len("noise32/"):]: GATE_FACTOR * (g[k] + g["perturb/" + k[len("noise32/"):]]) for k in g.files
            if k.startswith("noise32/")}


def worst(got, ref, gate):
    """(largest m / gate over both forms, the tensor it is at) over every tensor of ``ref``."""
    assert set(got) == set(ref) == set(gate), sorted(set(got) ^ set(ref))
    q = {k: float(np.max(metric(got[k], ref[k]) / gate[k])) for k in ref}
    k = max(q, key=q.get)
    return q[k], k, q
