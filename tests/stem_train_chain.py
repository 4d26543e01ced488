"""The stem and layer1..4 under train() as one chain from the image: conv1, bn1, ReLU, max-pool
(models/fpn_resnet.py:179-182) and the eight BasicBlocks (:184-187), all 20 BatchNorms on batch statistics, restated in
torch ops (F.conv2d, F.batch_norm(training=True), F.max_pool2d) and differentiated by autograd, built as
tests/block_train_chain.py builds its chain (its state, cotangents, metric and gate form are reused).  The loss is
L = sum_L <g_L, out_layer_L>, so x and every one of the 60 parameters get a gradient.

The composed gate is §28's / §32's: gate(t) = GATE_FACTOR (noise32(t) + perturb(t)) in both forms of
chain_restatement.metric; noise32 is the float32 CPU run of this very chain against the float64 one, perturb the
float64 chain with every stage (each convolution's, each BatchNorm's and the pool's output) moved by
GATE max(1, |v|) U(-1, 1).  tests/golden/gen_stem_train_chain_golden.py measures both on the CPU and stores them with
the conditioned image: every pre-activation and every pool window's lead at least MARGIN."""
import numpy as np
import torch
import torch.nn.functional as F

import block_train_chain as bc
import block_train_restatement as tr
import stem_train_restatement as st
from block_train_chain import GATE, GATE_FACTOR, GATE_LIMIT, LAYERS, MARGIN, cotangents, gates, metric, tensors, worst  # noqa: F401

SHAPE = (2, 3, 64, 96)
STEM_SEED = 760
MUTANTS = ("stem_running_stats", "no_skip_grad", "bn1_no_xhat")


def draw_state():
    """block_train_chain.draw_state() with the stem's conv1.weight and bn1 entries in front."""
    p = st.draw_params(STEM_SEED)
    sd = {"conv1.weight": p["conv1"]}
    for k, v in zip(("weight", "bias", "running_mean", "running_var"), p["bn1"]):
        sd["bn1." + k] = v
    sd.update(bc.draw_state())
    return sd


parameter_names = bc.parameter_names


def _pool_lead(a):
    B, C, oh, ow = a.shape
    top = F.unfold(a, 3, 1, 1, 2).reshape(B, C, 9, -1).topk(2, 2).values
    return torch.where(top[:, :, 0] > 0, top[:, :, 0] - top[:, :, 1], torch.ones_like(top[:, :, 0]))


@torch.enable_grad()  # whatever the process-wide switch is at
def forward_backward(state, x, dtype=torch.float64, perturb=None, mutant=None, want_pre=False):
    """(outs, grads, running, margin): the four maps, the gradients of L at "x" and the 60 parameters, the 40 running
    buffers after the step, and (``want_pre``) the smaller of the smallest |pre-activation| and the smallest pool lead."""
    P = {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in state.items()}
    for k in parameter_names(state):
        P[k].requires_grad_(True)
    xt = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    low = [np.inf]

    def stage(v):
        if perturb is None:
            return v
        noise = torch.from_numpy(perturb.uniform(-1.0, 1.0, tuple(v.shape))).to(dtype)
        return v + GATE * torch.clamp(v.detach().abs(), min=1.0) * noise

    def bn(v, pre):
        rm, rv, w, b = P[pre + ".running_mean"], P[pre + ".running_var"], P[pre + ".weight"], P[pre + ".bias"]
        if pre == "bn1" and mutant == "stem_running_stats":
            return stage(F.batch_norm(v, rm, rv, w, b, False, tr.MOMENTUM, tr.EPS))
        if pre == "bn1" and mutant == "bn1_no_xhat":
            F.batch_norm(v.detach(), rm, rv, None, None, True, tr.MOMENTUM, tr.EPS)  # moves the buffers
            return stage(bc._DropXhat.apply(v, tr.EPS) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1))
        return stage(F.batch_norm(v, rm, rv, w, b, True, tr.MOMENTUM, tr.EPS))

    def relu(v):
        if want_pre:
            low[0] = min(low[0], float(v.detach().abs().min()))
        return F.relu(v)

    a = relu(bn(stage(F.conv2d(xt, P["conv1.weight"], stride=2, padding=3)), "bn1"))
    if want_pre:
        low[0] = min(low[0], float(_pool_lead(a.detach()).min()))
    outs, t = [], stage(F.max_pool2d(a, 3, 2, 1))
    for L, b in bc.BLOCKS:
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
    return {n: o.detach().numpy() for n, o in zip(LAYERS, outs)}, grads, running, low[0]


def condition_image(state, x, margin=MARGIN, steps=4000, rate=2e-4):
    """x moved by gradient descent on sum max(0, 2 margin - |v|) over every pre-activation and the stem's pool leads
    until the float32 rounding of it has all of them at least ``margin`` (block_train_chain.condition_input's scheme)."""
    D = torch.float64
    P = {k: torch.from_numpy(np.asarray(v)).to(D) for k, v in state.items()}
    bn = lambda v, k: F.batch_norm(v, None, None, P[k + ".weight"], P[k + ".bias"], True, 0.0, tr.EPS)  # noqa: E731
    x = np.asarray(x, np.float64)
    for it in range(steps):
        x32 = x.astype(np.float32)
        if it % 5 == 0 and forward_backward(state, x32, want_pre=True)[3] >= margin:
            return x32
        with torch.enable_grad():
            xt = torch.from_numpy(x).requires_grad_(True)
            _condition_loss(P, bn, xt, margin).backward()
        x = x - rate * min(6.0, 1.0 + it / 40.0) * xt.grad.numpy()
    raise RuntimeError("condition_image: the margin was not reached")


def _condition_loss(P, bn, xt, margin):
    """The hinge over every pre-activation and the stem's pool leads that condition_image() descends."""
    p0 = bn(F.conv2d(xt, P["conv1.weight"], stride=2, padding=3), "bn1")
    a = F.relu(p0)
    pres, t = [p0, _pool_lead(a)], F.max_pool2d(a, 3, 2, 1)
    for L, b in bc.BLOCKS:
        pre = f"layer{L}.{b}"
        ds = pre + ".downsample.0.weight" in P
        s = 2 if ds else 1
        p1 = bn(F.conv2d(t, P[pre + ".conv1.weight"], stride=s, padding=1), pre + ".bn1")
        z = bn(F.conv2d(F.relu(p1), P[pre + ".conv2.weight"], padding=1), pre + ".bn2")
        p2 = z + (bn(F.conv2d(t, P[pre + ".downsample.0.weight"], stride=s), pre + ".downsample.1") if ds else t)
        pres += [p1, p2]
        t = F.relu(p2)
    return sum(F.relu(2 * margin - v.abs()).sum() for v in pres)
