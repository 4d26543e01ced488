"""Drop-in for the reference's models/fpn_resnet.py — KFPN ResNet on gfx950.

The module tree mirrors the reference's registration order exactly
(fpn_resnet.py:42-53 BasicBlock, :114-151 PoseResNet, heads in sorted() order
:135) so ``load_state_dict`` accepts the reference's 186-entry checkpoints and
``state_dict()`` round-trips them.  The submodules are parameter containers
only: ``PoseResNet.forward`` packs them (BatchNorm folded, OHWI layout) into one
device buffer on first use / after any parameter change, and runs the whole
forward — stem, 8 BasicBlocks, FPN, 15 heads, KFPN softmax — as HIP kernels
(libsfa_hip.so).  There is no CPU path: a CPU input raises ``SfaNativeError``.

Deviation (documented in DESIGN.md): the reference's per-forward visualisation
copies (fpn_resnet.py:189-242, ≈41 MB/frame) are opt-in through
``capture_visualization = True``.
"""

from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from sfa_hip import _lib
from sfa_hip import dropin as _dropin
from sfa_hip.runtime import (KfpnEngine, block_train_forward, block_train_grad, bn_unfold_grad, kfpn_combine_grad, kfpn_heads,
                             device_packable, pack_state_dict, state_entries, stem_train_forward, stem_train_grad)

BN_MOMENTUM = 0.1

# Generation of the module structure of the process: bumped whenever any module registers a
# parameter, buffer or submodule (torch's global registration hooks) and when PoseResNet._apply
# swaps tensors, so PoseResNet can keep its list of state tensors between forwards and re-walk
# state_dict() only when the structure may have changed (a state_dict walk is ~1.1 ms of host
# time per forward, the cached list's (data_ptr, _version) check ~40 us).
_STRUCT_GEN = [0]


def _bump_struct_gen(*_args, **_kw):
    _STRUCT_GEN[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_bump_struct_gen)
torch.nn.modules.module.register_module_buffer_registration_hook(_bump_struct_gen)
torch.nn.modules.module.register_module_module_registration_hook(_bump_struct_gen)

# Private switch of the tests and the timing tool: False sends every weight change through the host pack
# (pack_state_dict + a new engine), the route a model whose state is not float32 on the GPU always takes.
_DEVICE_REPACK = [True]

model_urls = {
    "resnet18": "https://download.pytorch.org/models/resnet18-5c106cde.pth",
}


def conv3x3(in_planes, out_planes, stride=1):
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)


class BasicBlock(nn.Module):
    """Parameter container of fpn_resnet.py:42-71 (executed fused by the HIP forward)."""

    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes, momentum=BN_MOMENTUM)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes, momentum=BN_MOMENTUM)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        raise RuntimeError("BasicBlock runs fused inside PoseResNet's HIP forward")


def _trainable_forward(ctx, eng, in_layout, x):
    """The engine's forward into a workspace this call keeps for backward: the five maps in head order."""
    B, _, H, W = x.shape
    with torch.cuda.device(x.device):
        outs = eng.alloc_outputs(B, H, W)
        ws = torch.empty(eng.workspace_bytes(B, H, W), dtype=torch.uint8, device=x.device)
        eng.forward_into(x, outs, in_layout, ws)
    ctx.eng, ctx.ws, ctx.shape = eng, ws, (B, H, W)
    return tuple(outs[n] for n, _ in eng.heads)


def _trainable_backward(ctx, grads, neck_need=()):
    """sfa_kfpn_combine_grad, then sfa_model_heads_grad per level on the workspace's level maps and heads' inputs: the
    60 head gradients, level-major.  With any of ``neck_need`` (which of the six neck parameters want a gradient)
    also sfa_model_heads_input_grad per level on the dA that leaves, and sfa_model_neck_grad on those three gradients
    and the workspace's layer1..4, up_level2 and up_level3 maps: (the six neck gradients or Nones, the 60)."""
    eng, ws, (B, H, W) = ctx.eng, ctx.ws, ctx.shape
    neck = any(neck_need)
    with torch.cuda.device(ws.device):
        views = eng.debug_views(ws, B, H, W)
        levels = {n: [t.contiguous() for t in lv] for n, lv in views["levels"].items()}
        gout = {n: (g.contiguous() if g is not None else torch.zeros_like(levels[n][1]))
                for (n, _), g in zip(eng.heads, grads)}
        glev = kfpn_combine_grad(levels, gout, level0_half=True)
        flat, gx = [], []
        for level in range(3):
            res = eng.heads_param_grad(level, eng.level_input(ws, B, H, W, level),
                                       {n: glev[n][level] for n, _ in eng.heads}, want_hidden=neck)
            if neck:
                res, _, dA = res
                gx.append(eng.heads_input_grad(level, dA))
            for n, _ in eng.heads:
                flat += list(res[n])
        dp = [None] * 6
        if neck:
            nhwc = lambda k: views[k].permute(0, 2, 3, 1)  # noqa: E731
            _, dp = eng.neck_grad(*gx, layers=[nhwc(f"layer{i}") for i in (1, 2, 3, 4)],
                                  ups=[nhwc("up_level2"), nhwc("up_level3")], want_layers=(False,) * 4,
                                  want_params=tuple(neck_need))
    return list(dp), flat


class _TrainableHeadsForward(torch.autograd.Function):
    """PoseResNet.forward with the 60 head parameters as differentiable inputs (heads_trainable()).  forward is
    the engine's forward into a workspace this call keeps; backward takes the level maps and the heads' inputs
    from that workspace and runs sfa_kfpn_combine_grad, then sfa_model_heads_grad per level.  The input image
    gets no gradient (nothing behind the heads is differentiated)."""

    @staticmethod
    def forward(ctx, eng, in_layout, x, *params):
        ctx.save_for_backward(*params)  # the head weights backward reads again: a stale backward raises
        return _trainable_forward(ctx, eng, in_layout, x)

    @staticmethod
    def backward(ctx, *grads):
        _ = ctx.saved_tensors
        _, flat = _trainable_backward(ctx, grads)
        return (None, None, None) + tuple(t if need else None for t, need in zip(flat, ctx.needs_input_grad[3:]))


class _LevelHeads(torch.autograd.Function):
    """One KFPN level's heads as an operator over the level's input and its 20 head parameters: forward is
    sfa_model_heads_forward on ``x`` (NHWC view of a channels-last tensor), backward runs sfa_model_heads_grad
    (which recomputes the forward's own Hd, bit for bit) and sfa_model_heads_input_grad on the dA it leaves."""

    @staticmethod
    def forward(ctx, eng, level, x, *params):
        xn = x.permute(0, 2, 3, 1)
        with torch.cuda.device(x.device):
            ys = eng.heads_forward(level, xn)
        ctx.eng, ctx.level = eng, level
        ctx.save_for_backward(xn, *params)
        return tuple(ys[n] for n, _ in eng.heads)

    @staticmethod
    def backward(ctx, *grads):
        eng, level, xn = ctx.eng, ctx.level, ctx.saved_tensors[0]
        B, h, w, _ = xn.shape
        with torch.cuda.device(xn.device):
            g = {n: (gr.contiguous() if gr is not None else torch.zeros((B, c, h, w), device=xn.device))
                 for (n, c), gr in zip(eng.heads, grads)}
            res, _, dA = eng.heads_param_grad(level, xn, g, want_hidden=True)
            dx = eng.heads_input_grad(level, dA).permute(0, 3, 1, 2) if ctx.needs_input_grad[2] else None
        flat = [t for n, _ in eng.heads for t in res[n]]
        return (None, None, dx) + tuple(t if need else None for t, need in zip(flat, ctx.needs_input_grad[3:]))


def _nhwc_grad(g, shape, device):
    """An upstream NCHW gradient as a contiguous NHWC tensor (zeros for None)."""
    if g is None:
        return torch.zeros(shape, dtype=torch.float32, device=device)
    return g.permute(0, 2, 3, 1).contiguous()


class _NeckFromLayers(torch.autograd.Function):
    """The FPN neck as an operator over the four backbone maps and the six conv_up_level parameters: forward is
    sfa_model_neck_forward on the NHWC views of channels-last tensors, backward one sfa_model_neck_grad for the
    inputs that require grad (the operator is linear: besides the maps its convolutions read, nothing is saved)."""

    @staticmethod
    def forward(ctx, eng, l1, l2, l3, l4, *params):
        ls = [t.permute(0, 2, 3, 1) for t in (l1, l2, l3, l4)]
        with torch.cuda.device(l4.device):
            u2, u3, u4 = eng.neck_forward(*ls)
        ctx.eng = eng
        ctx.save_for_backward(*ls, u2, u3, *params)
        return tuple(t.permute(0, 3, 1, 2) for t in (u2, u3, u4))

    @staticmethod
    def backward(ctx, g2, g3, g4):
        eng = ctx.eng
        l1, l2, l3, l4, u2, u3 = ctx.saved_tensors[:6]
        need = ctx.needs_input_grad
        if not any(need[1:]):
            return (None,) * len(need)
        with torch.cuda.device(l4.device):
            g4 = _nhwc_grad(g4, l1.shape, l4.device)
            g2, g3 = (None if g is None else _nhwc_grad(g, None, None) for g in (g2, g3))
            dl, dp = eng.neck_grad(g2, g3, g4, layers=(l1, l2, l3, l4), ups=(u2, u3), want_layers=need[1:5],
                                   want_params=need[5:11])
        return (None,) + tuple(None if t is None else t.permute(0, 3, 1, 2) for t in dl) + tuple(dp)


class _BlockFromInput(torch.autograd.Function):
    """One BasicBlock as an operator over its input and its 6 (9 with a downsample) parameters: forward is
    sfa_model_block_forward on the NHWC view of a channels-last tensor, BatchNorm folded with the running statistics;
    backward one sfa_model_block_grad on the saved x, mid and y, then sfa_bn_unfold_grad per convolution.  ``mods``:
    the (conv, bn) pairs conv1 / bn1, conv2 / bn2 and, with a downsample, downsample.0 / downsample.1; ``params``:
    their weight, bn.weight, bn.bias in that order."""

    @staticmethod
    def forward(ctx, eng, layer, block, mods, x, *params):
        xn = x.permute(0, 2, 3, 1)
        with torch.cuda.device(x.device):
            mid, y = eng.block_forward(layer, block, xn)
        ctx.eng, ctx.layer, ctx.block, ctx.mods = eng, layer, block, mods
        ctx.save_for_backward(xn, mid, y, *params, *[t for _, bn in mods for t in (bn.running_mean, bn.running_var)])
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        eng, mods = ctx.eng, ctx.mods
        xn, mid, y = ctx.saved_tensors[:3]
        need = ctx.needs_input_grad
        pneed = [need[5 + 3 * i:8 + 3 * i] for i in range(len(mods))]
        if not need[4] and not any(any(n) for n in pneed):
            return (None,) * len(need)
        with torch.cuda.device(xn.device):
            g = _nhwc_grad(gy, y.shape, xn.device)
            # dW' of conv i feeds its dW and dgamma, db' its dgamma and dbeta; the downsample's db' is conv2's
            want = [False] * 5
            for i, n in enumerate(pneed):
                want[(0, 2, 4)[i]] = n[0] or n[1]
                want[(1, 3, 3)[i]] = want[(1, 3, 3)[i]] or n[1] or n[2]
            dx, dp = eng.block_grad(ctx.layer, ctx.block, xn, mid, y, g, want_x=need[4], want_params=want)
            out = []
            for i, ((conv, bn), n) in enumerate(zip(mods, pneed)):
                if not any(n):
                    out += [None, None, None]
                    continue
                out += list(bn_unfold_grad(conv.weight, bn.weight, bn.running_mean, bn.running_var, bn.eps,
                                           dp[(0, 2, 4)[i]] if (n[0] or n[1]) else torch.empty_like(conv.weight),
                                           dp[(1, 3, 3)[i]] if (n[1] or n[2]) else torch.empty_like(bn.weight), want=n))
        return (None, None, None, None, None if dx is None else dx.permute(0, 3, 1, 2)) + tuple(out)


class _BlockTrainFromInput(torch.autograd.Function):
    """One BasicBlock in training mode as an operator over its input and its 6 (9 with a downsample) parameters:
    forward is sfa_block_train_forward on the NHWC view of a channels-last tensor and the raw parameters, every
    BatchNorm normalising with the statistics of the batch; backward one sfa_block_train_grad on the saved maps and
    statistics, every BatchNorm differentiated through them.  No engine and no host repack.  Returns (y, stats);
    ``stats`` (nbn, 2, Cout), the batch means and biased variances, is not differentiable."""

    @staticmethod
    def forward(ctx, layer, block, eps, x, *params):
        xn = x.permute(0, 2, 3, 1)
        ps = [p.detach().contiguous() for p in params]
        with torch.cuda.device(x.device):
            m = block_train_forward(layer, block, xn, ps, eps)
        ctx.layer, ctx.block, ctx.eps, ctx.ds = layer, block, eps, m["zd"] is not None
        ctx.save_for_backward(xn, m["z1"], m["mid"], m["z2"], m["y"], m["stats"], *([m["zd"]] if ctx.ds else []), *ps)
        ctx.mark_non_differentiable(m["stats"])
        return m["y"].permute(0, 3, 1, 2), m["stats"]

    @staticmethod
    def backward(ctx, gy, _gstats):
        saved = ctx.saved_tensors
        xn, z1, mid, z2, y, stats = saved[:6]
        zd = saved[6] if ctx.ds else None
        ps = list(saved[7 if ctx.ds else 6:])
        need = ctx.needs_input_grad
        if not any(need[3:]):
            return (None,) * len(need)
        with torch.cuda.device(xn.device):
            g = _nhwc_grad(gy, y.shape, xn.device)
            dx, dp = block_train_grad(ctx.layer, ctx.block, xn, dict(z1=z1, mid=mid, z2=z2, zd=zd, y=y, stats=stats), g,
                                      ps, ctx.eps, want_x=need[3], want_params=need[4:])
        return (None, None, None, None if dx is None else dx.permute(0, 3, 1, 2)) + tuple(dp[:len(ps)])


class _StemFromImage(torch.autograd.Function):
    """The stem as an operator over the image and conv1.weight, bn1.weight, bn1.bias: forward is sfa_model_stem_forward,
    BatchNorm folded with the running statistics; backward one sfa_model_stem_grad on the saved x and a (the pool's
    window maxima are recomputed from a), then sfa_bn_unfold_grad on conv1 / bn1.  The image gradient is computed only
    when the image requires grad."""

    @staticmethod
    def forward(ctx, eng, conv, bn, x, *params):
        with torch.cuda.device(x.device):
            a, pooled = eng.stem_forward(x)
        ctx.eng, ctx.conv, ctx.bn = eng, conv, bn
        ctx.save_for_backward(x, a, *params, bn.running_mean, bn.running_var)
        return pooled.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gp):
        eng, conv, bn = ctx.eng, ctx.conv, ctx.bn
        x, a = ctx.saved_tensors[:2]
        need = ctx.needs_input_grad
        n = need[4:7]
        if not need[3] and not any(n):
            return (None,) * len(need)
        with torch.cuda.device(x.device):
            B, oh, ow, _ = a.shape
            g = _nhwc_grad(gp, (B, -(-oh // 2), -(-ow // 2), 64), x.device)
            # dW' feeds dW and dgamma, db' dgamma and dbeta
            want = (n[0] or n[1], n[1] or n[2])
            dx, dp = eng.stem_grad(x, a, g, want_x=need[3], want_params=want)
            out = [None, None, None]
            if any(n):
                out = list(bn_unfold_grad(conv.weight, bn.weight, bn.running_mean, bn.running_var, bn.eps,
                                          dp[0] if want[0] else torch.empty_like(conv.weight),
                                          dp[1] if want[1] else torch.empty_like(bn.weight), want=n))
        return (None, None, None, dx) + tuple(out)


class _StemTrainFromImage(torch.autograd.Function):
    """The stem in training mode as an operator over the image and conv1.weight, bn1.weight, bn1.bias: forward is
    sfa_stem_train_forward on the raw parameters, bn1 normalising with the statistics of the batch; backward one
    sfa_stem_train_grad on the saved x, z, a and statistics, bn1 differentiated through them.  No engine and no host
    repack.  Returns (pooled, stats); ``stats`` (2, 64), the batch mean and biased variance, is not differentiable."""

    @staticmethod
    def forward(ctx, eps, x, *params):
        ps = [p.detach().contiguous() for p in params]
        with torch.cuda.device(x.device):
            m = stem_train_forward(x, ps, eps)
        ctx.eps = eps
        ctx.save_for_backward(x, m["z"], m["a"], m["stats"], *ps)
        ctx.mark_non_differentiable(m["stats"])
        return m["pooled"].permute(0, 3, 1, 2), m["stats"]

    @staticmethod
    def backward(ctx, gp, _gstats):
        x, z, a, stats = ctx.saved_tensors[:4]
        ps = list(ctx.saved_tensors[4:])
        need = ctx.needs_input_grad
        if not any(need[1:]):
            return (None,) * len(need)
        with torch.cuda.device(x.device):
            B, oh, ow, _ = a.shape
            g = _nhwc_grad(gp, (B, -(-oh // 2), -(-ow // 2), 64), x.device)
            dx, dp = stem_train_grad(x, dict(z=z, a=a, stats=stats), g, ps, ctx.eps, want_x=need[1], want_params=need[2:5])
        return (None, dx) + tuple(dp)


class _TrainableNeckForward(torch.autograd.Function):
    """PoseResNet.forward with the 6 neck and the 60 head parameters as differentiable inputs (neck_trainable()):
    _TrainableHeadsForward one stage deeper (_trainable_backward with the neck's part).  The input image and the
    backbone get no gradient."""

    @staticmethod
    def forward(ctx, eng, in_layout, x, *params):
        # the head weights and, through sfa_model_neck_grad's data gradients, the neck convs' weights are read again
        ctx.save_for_backward(*params)
        return _trainable_forward(ctx, eng, in_layout, x)

    @staticmethod
    def backward(ctx, *grads):
        _ = ctx.saved_tensors
        need = ctx.needs_input_grad[3:]
        dp, flat = _trainable_backward(ctx, grads, need[:6])
        return (None, None, None) + tuple(t if n else None for t, n in zip(dp + flat, need))


class PoseResNet(nn.Module):
    def __init__(self, block, layers, heads, head_conv, **kwargs):
        self.inplanes = 64
        self.deconv_with_bias = False
        self.heads = heads
        super().__init__()
        if block is not BasicBlock or list(layers) != [2, 2, 2, 2]:
            raise NotImplementedError("the HIP forward implements fpn_resnet_18 (BasicBlock x [2,2,2,2])")
        if head_conv != 64:
            raise NotImplementedError("the HIP forward implements head_conv = 64")
        self.head_conv = head_conv
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64, momentum=BN_MOMENTUM)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.conv_up_level1 = nn.Conv2d(768, 256, kernel_size=1, stride=1, padding=0)
        self.conv_up_level2 = nn.Conv2d(384, 128, kernel_size=1, stride=1, padding=0)
        self.conv_up_level3 = nn.Conv2d(192, 64, kernel_size=1, stride=1, padding=0)
        for fpn_idx, fpn_c in enumerate([256, 128, 64]):
            for head in sorted(self.heads):
                self.__setattr__(f"fpn{fpn_idx}_{head}", nn.Sequential(
                    nn.Conv2d(fpn_c, head_conv, kernel_size=3, padding=1, bias=True),
                    nn.ReLU(inplace=True),
                    nn.Conv2d(head_conv, self.heads[head], kernel_size=1, stride=1, padding=0)))
        # visualisation attributes (fpn_resnet.py:147-151); filled only when opted in
        self.capture_visualization = False
        self.kfpn_features = []
        self.fpn_outputs = {}
        self.kfpn_weights = {}
        self.backbone_features = {}
        self._arch = _lib.make_arch(dict(self.heads), head_conv)
        self._engines = {}
        self._math = None  # set_math: None = the engine's default (SFA_MATH or fp16x3)
        self._sig = None
        self._state_tensors = None  # (structure generation, [state tensors]) cache of _signature
        self._heads_trainable = False
        self._neck_trainable = False
        self._backbone_trainable = False
        self._backbone_batch_stats = False

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion, momentum=BN_MOMENTUM))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    # -------------------------------------------------------------- engine
    def _signature(self):
        """(data_ptr, version) of every state tensor: any in-place update, reload or move of a
        parameter changes it, and the engine repacks the weights."""
        cache = self._state_tensors
        if cache is None or cache[0] != _STRUCT_GEN[0]:
            cache = self._state_tensors = (_STRUCT_GEN[0], list(self.state_dict(keep_vars=True).values()))
        return tuple((t.data_ptr(), t._version) for t in cache[1])

    def _apply(self, fn, *args, **kw):  # .to() / .cuda() / .float() may replace the tensors
        out = super()._apply(fn, *args, **kw)
        _bump_struct_gen()
        return out

    def _device_route(self, tensors, device) -> bool:
        return _DEVICE_REPACK[0] and len(tensors) == state_entries(self._arch) and device_packable(tensors, device)

    def _engine(self, device) -> KfpnEngine:
        """The engine of ``device``.  When only values changed since the last call (the same structure, every
        data_ptr unchanged, new versions) and the state is contiguous float32 on the engine's device, the live
        engine is repacked in place on the current stream (KfpnEngine.repack) and stays the same object: its
        options, workspaces, twins and captured graphs survive an optimiser step.  Anything else (a CPU-resident
        model, another dtype, a moved or re-registered tensor) drops the engines and packs on the host."""
        walked = self._state_tensors
        sig = self._signature()
        tensors = self._state_tensors[1]
        if sig != self._sig:
            # nothing is kept while a repack can still fail: an exception leaves no engine and no signature, so the
            # next call packs again from scratch instead of returning half-written weights
            old, engines = self._sig, self._engines
            self._sig, self._engines = None, {}
            same_tensors = walked is self._state_tensors or (
                walked is not None and len(walked[1]) == len(tensors) and all(a is b for a, b in zip(walked[1], tensors)))
            keep = (old is not None and same_tensors and len(old) == len(sig)
                    and all(a[0] == b[0] for a, b in zip(old, sig)))
            live = {}
            for dev, eng in (engines.items() if keep else ()):
                if self._device_route(tensors, dev):
                    live[dev] = eng.repack(tensors)
            self._sig, self._engines = sig, live
        eng = self._engines.get(device)
        if eng is None:
            if self._device_route(tensors, device):
                eng = KfpnEngine.from_state(self._arch, tensors, device, math=self._math)
            else:
                packed = pack_state_dict(self.state_dict(), self._arch)
                eng = KfpnEngine(self._arch, packed, device, math=self._math)
            self._engines[device] = eng
        return eng

    def set_math(self, math):
        """Convolution arithmetic of this model's forwards: "fp16x3" (the default), "bf16x6", "f32" or the
        opt-in reduced-precision "fp16" (one fp16 product per MAC in the residual layers and the heads: faster,
        logit error ~1e-3 instead of <= 1e-5; include/sfa_hip.h sfa_math), or the _lib.MATH_* integer.
        Applies to the engines this model already has and to every one it creates later."""
        if isinstance(math, str):
            if math.strip().lower() not in _lib.MATH_NAMES:
                raise ValueError(f"set_math({math!r}): expected one of {sorted(_lib.MATH_NAMES)}")
            math = _lib.MATH_NAMES[math.strip().lower()]
        math = int(math)
        if math not in _lib.MATH_NAMES.values():
            raise ValueError(f"set_math({math}): expected one of {sorted(_lib.MATH_NAMES.values())}")
        for eng in self._engines.values():
            eng.set_math(math)
        self._math = math

    def forward(self, x):
        return self.forward_layout(x, _lib.IN_NCHW3)

    def heads_trainable(self, flag=True):
        """Fine-tuning of the detection heads on a frozen backbone.  Off (the default): forward runs under
        no_grad and returns detached maps.  On: with grad mode enabled, forward returns the same five maps (bit
        for bit) carrying a grad_fn whose backward leaves ``.grad`` at the 60 head parameters
        ``fpn{0,1,2}_{head}.{0,2}.{weight,bias}`` that require grad (sfa_kfpn_combine_grad, then
        sfa_model_heads_grad per level).  Nothing behind the heads is differentiated: the input and every other
        parameter get no gradient, and BatchNorm stays folded with its running statistics.  A batch above one
        forward pass (``max_batch``) is refused in this mode.  Returns self."""
        self._heads_trainable = bool(flag)
        return self

    def head_parameters(self):
        """The 60 head parameters in the order the trainable forward differentiates them: level, head (forward
        order), then 0.weight, 0.bias, 2.weight, 2.bias."""
        out = []
        for f in range(3):
            for head in self.heads:
                seq = getattr(self, f"fpn{f}_{head}")
                out += [seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias]
        return out

    def level_heads(self, level, x):
        """The heads of KFPN ``level`` (0, 1, 2: ``fpn{level}_{head}``, Cin 256 / 128 / 64) on a caller's feature map
        ``x``, a (B, Cin, h, w) float32 GPU tensor taken as channels-last bytes (a channels-last producer costs no
        copy): {head: (B, c, h, w)}.  Differentiable with respect to ``x`` and the level's 20 head parameters
        (sfa_model_heads_forward; sfa_model_heads_grad and sfa_model_heads_input_grad in backward), so a torch-built
        backbone and neck can sit under the HIP heads and train.  Parameters that do not require grad get None."""
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise _lib.SfaNativeError("PoseResNet.level_heads runs on the GPU (HIP) only")
        if level not in (0, 1, 2) or x.dim() != 4 or x.shape[1] != _lib.HEADS_LEVEL_CIN[level]:
            raise ValueError(f"level_heads: expected (B, {_lib.HEADS_LEVEL_CIN[level] if level in (0, 1, 2) else '?'}, "
                             f"h, w) at level {level!r}, got {tuple(x.shape)}")
        eng = self._engine(x.device)
        x = x.float().contiguous(memory_format=torch.channels_last)
        params = self.head_parameters()[20 * level:20 * level + 20]
        res = _LevelHeads.apply(eng, int(level), x, *params)
        return {n: t for (n, _), t in zip(eng.heads, res)}

    def heads_from_levels(self, up_level2, up_level3, up_level4):
        """The loop of models/fpn_resnet.py:219-244 on a caller's three level inputs (B, 256, h / 2, w / 2),
        (B, 128, h, w), (B, 64, h, w): :meth:`level_heads` per level, then the KFPN combine (level 0 read at half
        resolution).  Returns the five maps {head: (B, c, h, w)} whose grad_fn reaches the three inputs and the 60
        head parameters."""
        per_level = [self.level_heads(f, x) for f, x in enumerate((up_level2, up_level3, up_level4))]
        return kfpn_heads({n: [lv[n] for lv in per_level] for n in per_level[0]}, level0_half=True)

    def neck_trainable(self, flag=True):
        """:meth:`heads_trainable` one stage deeper: fine-tuning of the FPN neck and the detection heads on a frozen
        backbone.  On, with grad mode enabled, forward returns the same five maps (bit for bit) carrying a grad_fn
        whose backward leaves ``.grad`` at ``conv_up_level{1,2,3}.{weight,bias}`` and at the 60 head parameters
        that require grad (sfa_kfpn_combine_grad, per level sfa_model_heads_grad and sfa_model_heads_input_grad, then
        sfa_model_neck_grad on the forward's own layer1..4, up_level2 and up_level3 maps).  The input image and the
        backbone get no gradient, and BatchNorm stays folded with its running statistics.  A batch above one forward
        pass (``max_batch``) is refused in this mode.  Returns self."""
        self._no_neck("neck_trainable")
        self._neck_trainable = bool(flag)
        return self

    def neck_parameters(self):
        """conv_up_level1.weight, .bias, conv_up_level2.weight, .bias, conv_up_level3.weight, .bias."""
        self._no_neck("neck_parameters")
        return [p for m in (self.conv_up_level1, self.conv_up_level2, self.conv_up_level3) for p in (m.weight, m.bias)]

    def _no_neck(self, what):
        if not hasattr(self, "conv_up_level1"):
            raise AttributeError(f"{what}: the plain resnet has no FPN neck (models/resnet.py)")

    def neck_from_layers(self, out_layer1, out_layer2, out_layer3, out_layer4):
        """Lines 197-210 of models/fpn_resnet.py on a caller's four backbone maps (B, 64, 8 h, 8 w), (B, 128, 4 h, 4 w),
        (B, 256, 2 h, 2 w), (B, 512, h, w), float32 GPU tensors taken as channels-last bytes (a channels-last producer
        costs no copy): returns (up_level2, up_level3, up_level4) = (B, 256, 4 h, 4 w), (B, 128, 8 h, 8 w),
        (B, 64, 8 h, 8 w).  Differentiable with respect to the four maps and the six neck parameters
        (sfa_model_neck_forward; sfa_model_neck_grad in backward); parameters that do not require grad get None.
        float32 MFMA arithmetic: not bit-equal to the model's own fused FPN stage."""
        self._no_neck("neck_from_layers")
        layers = (out_layer1, out_layer2, out_layer3, out_layer4)
        for i, t in enumerate(layers):
            if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
                raise _lib.SfaNativeError("PoseResNet.neck_from_layers runs on the GPU (HIP) only")
            if t.dim() != 4 or t.shape[1] != _lib.NECK_LAYER_C[i]:
                raise ValueError(f"neck_from_layers: out_layer{i + 1} is {tuple(t.shape)}, expected "
                                 f"(B, {_lib.NECK_LAYER_C[i]}, h, w)")
        B, _, h4, w4 = out_layer4.shape
        for i, t in enumerate(layers):
            want = (B, _lib.NECK_LAYER_C[i], h4 << (3 - i), w4 << (3 - i))
            if tuple(t.shape) != want:
                raise ValueError(f"neck_from_layers: out_layer{i + 1} is {tuple(t.shape)}, expected {want}")
        eng = self._engine(out_layer4.device)
        layers = [t.float().contiguous(memory_format=torch.channels_last) for t in layers]
        return _NeckFromLayers.apply(eng, *layers, *self.neck_parameters())

    def detect_from_layers(self, out_layer1, out_layer2, out_layer3, out_layer4):
        """The whole HIP detector top on a caller's four backbone maps: :meth:`heads_from_levels` of
        :meth:`neck_from_layers`.  The five maps {head: (B, c, 8 h, 8 w)} carry a grad_fn reaching the four maps and
        all 66 neck and head parameters."""
        return self.heads_from_levels(*self.neck_from_layers(out_layer1, out_layer2, out_layer3, out_layer4))

    def _block_mods(self, layer, block):
        blk = getattr(self, f"layer{layer}")[block]
        mods = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)]
        if blk.downsample is not None:
            mods.append((blk.downsample[0], blk.downsample[1]))
        return tuple(mods)

    def block_parameters(self):
        """The 57 parameters of the eight BasicBlocks in the order :meth:`block_from_input` differentiates them: layer,
        block, then conv1.weight, bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias and, on a block with a
        downsample, downsample.0.weight, downsample.1.weight, downsample.1.bias."""
        self._no_neck("block_parameters")
        return [p for L in (1, 2, 3, 4) for b in (0, 1) for conv, bn in self._block_mods(L, b)
                for p in (conv.weight, bn.weight, bn.bias)]

    def block_from_input(self, layer, block, x, batch_stats=False, update_running=True):
        """BasicBlock ``layer{layer}.{block}`` (models/fpn_resnet.py:42-71) on a caller's ``x``, a (B, Cin, h, w) float32
        GPU tensor taken as channels-last bytes: returns the block's output (B, Cout, ceil(h / s), ceil(w / s)).
        BatchNorm uses its running statistics whatever ``.training`` says, folded into the convolutions, exactly as
        :meth:`forward` does; the gradients are those of the block in ``eval()``.  Differentiable with respect to ``x``
        and the block's 6 parameters (9 with a downsample): sfa_model_block_forward; sfa_model_block_grad and
        sfa_bn_unfold_grad in backward.  Parameters that do not require grad get None.  x, mid and y are saved for
        backward.  A parameter changed in place is seen by the next call (the engine repacks).

        ``batch_stats=True`` is the block under ``model.train()`` instead: every BatchNorm normalises with the mean
        and biased variance of the batch and is differentiated through them (sfa_block_train_forward /
        sfa_block_train_grad on the raw parameters; the engine is not called, nothing is repacked on the host; B oh ow
        must be at least 2).  After the forward each BatchNorm's ``running_mean``, ``running_var`` (unbiased,
        n / (n - 1)) and ``num_batches_tracked`` move exactly as ``nn.BatchNorm2d`` moves them in ``train()``, under
        ``no_grad``, unless ``update_running`` is False."""
        self._no_neck("block_from_input")
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise _lib.SfaNativeError("PoseResNet.block_from_input runs on the GPU (HIP) only")
        cin = KfpnEngine.block_shape(layer, block)[0]
        if x.dim() != 4 or x.shape[1] != cin:
            raise ValueError(f"block_from_input: expected (B, {cin}, h, w) at layer{layer}.{block}, got {tuple(x.shape)}")
        mods = self._block_mods(layer, block)
        params = [p for conv, bn in mods for p in (conv.weight, bn.weight, bn.bias)]
        if batch_stats:
            return self._block_train(int(layer), int(block), mods, params, x, update_running)
        eng = self._engine(x.device)
        x = x.float().contiguous(memory_format=torch.channels_last)
        return _BlockFromInput.apply(eng, int(layer), int(block), mods, x, *params)

    def _block_train(self, layer, block, mods, params, x, update_running):
        eps = float(mods[0][1].eps)
        if any(float(bn.eps) != eps for _, bn in mods):
            raise ValueError(f"block_from_input: the BatchNorms of layer{layer}.{block} differ in eps")
        x = x.float().contiguous(memory_format=torch.channels_last)
        y, stats = _BlockTrainFromInput.apply(layer, block, eps, x, *params)
        if update_running:
            n = y.numel() // y.shape[1]
            with torch.no_grad():
                for i, (_, bn) in enumerate(mods):
                    if bn.running_mean is None:
                        continue
                    bn.num_batches_tracked += 1
                    m = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else float(bn.momentum)
                    bn.running_mean.mul_(1.0 - m).add_(stats[i, 0], alpha=m)
                    bn.running_var.mul_(1.0 - m).add_(stats[i, 1], alpha=m * n / (n - 1))
        return y

    def layers_from_pooled(self, x, batch_stats=False, update_running=True):
        """``layer1..4`` (models/fpn_resnet.py:184-187) on a caller's pooled stem output ``x`` (B, 64, h, w): the eight
        blocks chained through :meth:`block_from_input` (``batch_stats`` / ``update_running`` as there).  Returns
        (out_layer1, out_layer2, out_layer3, out_layer4) whose grad_fn reaches ``x`` and the 57
        :meth:`block_parameters`."""
        kw = dict(batch_stats=True, update_running=update_running) if batch_stats else {}
        outs = []
        for layer in (1, 2, 3, 4):
            for block in (0, 1):
                x = self.block_from_input(layer, block, x, **kw)
            outs.append(x)
        return tuple(outs)

    def detect_from_pooled(self, x, batch_stats=False, update_running=True):
        """:meth:`detect_from_layers` of :meth:`layers_from_pooled`: everything behind the stem on a caller's pooled map
        (B, 64, h, w), h and w multiples of 8.  The five maps carry a grad_fn reaching ``x`` and 123 of the model's 126
        parameters; the stem's conv1.weight, bn1.weight, bn1.bias are reached through :meth:`detect_from_image`.
        ``batch_stats=True`` runs the eight blocks on batch statistics (the neck and the heads have no BatchNorm)."""
        return self.detect_from_layers(*self.layers_from_pooled(x, batch_stats=batch_stats, update_running=update_running))

    def stem_parameters(self):
        """conv1.weight, bn1.weight, bn1.bias: the order :meth:`stem_from_image` differentiates them in."""
        self._no_neck("stem_parameters")
        return [self.conv1.weight, self.bn1.weight, self.bn1.bias]

    def stem_from_image(self, x, batch_stats=False, update_running=True):
        """The stem (models/fpn_resnet.py:179-182: conv1, bn1, ReLU, max-pool) on a caller's image ``x``, a (B, 3, H, W)
        float32 GPU tensor: returns the pooled map (B, 64, ceil(H / 4), ceil(W / 4)) as channels-last bytes.  BatchNorm
        uses its running statistics whatever ``.training`` says, folded into conv1, exactly as :meth:`forward` does; the
        gradients are those of the stem in ``eval()``.  Differentiable with respect to ``x`` and the three
        :meth:`stem_parameters` (sfa_model_stem_forward; sfa_model_stem_grad and sfa_bn_unfold_grad in backward);
        parameters that do not require grad get None, and the image gradient is computed only when ``x`` requires
        grad.  x and the ReLU map are saved for backward.  The plain resnet family (models/resnet.py) refuses this
        method although the C entries accept its handles.

        ``batch_stats=True`` is the stem under ``model.train()`` instead: bn1 normalises with the mean and biased
        variance of the batch and is differentiated through them (sfa_stem_train_forward / sfa_stem_train_grad on the
        raw parameters, conv1 in float32; the engine is not called, nothing is repacked on the host; B oh ow must be at
        least 2).  After the forward ``bn1.running_mean``, ``running_var`` (unbiased, n / (n - 1)) and
        ``num_batches_tracked`` move exactly as ``nn.BatchNorm2d`` moves them in ``train()``, under ``no_grad``, unless
        ``update_running`` is False."""
        self._no_neck("stem_from_image")
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise _lib.SfaNativeError("PoseResNet.stem_from_image runs on the GPU (HIP) only")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"stem_from_image: expected (B, 3, H, W), got {tuple(x.shape)}")
        if batch_stats:
            return self._stem_train(x, update_running)
        eng = self._engine(x.device)
        x = x.float().contiguous()
        return _StemFromImage.apply(eng, self.conv1, self.bn1, x, *self.stem_parameters())

    def _stem_train(self, x, update_running):
        bn = self.bn1
        x = x.float().contiguous()
        pooled, stats = _StemTrainFromImage.apply(float(bn.eps), x, *self.stem_parameters())
        if update_running and bn.running_mean is not None:
            n = x.shape[0] * (-(-x.shape[2] // 2)) * (-(-x.shape[3] // 2))
            with torch.no_grad():
                bn.num_batches_tracked += 1
                m = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else float(bn.momentum)
                bn.running_mean.mul_(1.0 - m).add_(stats[0], alpha=m)
                bn.running_var.mul_(1.0 - m).add_(stats[1], alpha=m * n / (n - 1))
        return pooled

    def detect_from_image(self, x, batch_stats=False, update_running=True):
        """:meth:`detect_from_pooled` of :meth:`stem_from_image`: the whole detector through the differentiable
        operators on an image (B, 3, H, W), H and W multiples of 32.  The five maps carry a grad_fn reaching ``x`` (when
        it requires grad) and all 126 parameters.  ``batch_stats=True`` runs all 20 BatchNorms (bn1 and the eight
        blocks') on batch statistics and moves their running buffers (``update_running``), as the reference's
        ``model.train()`` forward does."""
        if isinstance(x, torch.Tensor) and x.dim() == 4 and (x.shape[2] % 32 or x.shape[3] % 32):
            raise ValueError(f"detect_from_image: H and W must be multiples of 32, got {tuple(x.shape)}")
        if batch_stats:
            return self.detect_from_pooled(self.stem_from_image(x, batch_stats=True, update_running=update_running),
                                           batch_stats=True, update_running=update_running)
        return self.detect_from_pooled(self.stem_from_image(x))

    def backbone_trainable(self, flag=True, batch_stats=False):
        """Training of the whole detector: the deepest of the three trainable modes, it wins over
        :meth:`neck_trainable` and :meth:`heads_trainable`.  On, with grad mode enabled, ``forward(x)`` returns
        :meth:`detect_from_image` of ``x``: five maps whose backward leaves ``.grad`` at all 126 parameters that require
        grad and at ``x`` when it does.  These maps are the operators' (fp16x3 stem and blocks, float32 MFMA neck,
        saved activations), so they equal the fused forward only within the per-stage gate and not bit for bit.  The
        flipped input layout is refused in this mode, and BatchNorm stays folded with its running statistics.  Off, or
        under ``no_grad``, forward is exactly what it is without this mode.  ``batch_stats=True`` makes that forward
        ``detect_from_image(x, batch_stats=True)`` instead: all 20 BatchNorms on batch statistics with their running
        buffers moving, one training step as the reference's ``model.train()`` runs it (``.train()`` / ``.eval()``
        themselves change nothing here).  Returns self."""
        self._no_neck("backbone_trainable")
        self._backbone_trainable = bool(flag)
        self._backbone_batch_stats = bool(flag) and bool(batch_stats)
        return self

    def forward_layout(self, x, in_layout):
        """forward() with the input read as ``in_layout``: _lib.IN_NCHW3 (the reference's), or
        _lib.IN_NCHW3_FLIP_HW = forward(torch.flip(x, [2, 3])) with the flip fused in."""
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise _lib.SfaNativeError("PoseResNet.forward runs on the GPU (HIP) only; move the "
                                      "model input to a GPU device")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected (B, 3, H, W), got {tuple(x.shape)}")
        if in_layout not in (_lib.IN_NCHW3, _lib.IN_NCHW3_FLIP_HW):
            raise ValueError(f"unsupported input layout {in_layout}")
        if self._backbone_trainable and torch.is_grad_enabled():
            if in_layout != _lib.IN_NCHW3:
                raise ValueError("backbone_trainable: the flipped input layout is not differentiated; flip the image")
            res = self.detect_from_image(x, batch_stats=True) if self._backbone_batch_stats else self.detect_from_image(x)
            self.kfpn_features, self.fpn_outputs = [], {}
            self.kfpn_weights, self.backbone_features = {}, {}
            return res
        eng = self._engine(x.device)
        x = x.contiguous().float()
        if (self._neck_trainable or self._heads_trainable) and torch.is_grad_enabled():
            B, _, H, W = x.shape
            mode = "neck_trainable" if self._neck_trainable else "heads_trainable"
            if B > eng.max_batch(H, W):
                raise ValueError(f"{mode}: batch {B} is above one forward pass ({eng.max_batch(H, W)} frames "
                                 f"at {H}x{W}); the workspace holds one pass only")
            if self._neck_trainable:
                res = _TrainableNeckForward.apply(eng, in_layout, x.detach(), *self.neck_parameters(),
                                                  *self.head_parameters())
            else:
                res = _TrainableHeadsForward.apply(eng, in_layout, x.detach(), *self.head_parameters())
            self.kfpn_features, self.fpn_outputs = [], {}
            self.kfpn_weights, self.backbone_features = {}, {}
            return {n: t for (n, _), t in zip(eng.heads, res)}
        with torch.no_grad(), torch.cuda.device(x.device):
            B, _, H, W = x.shape
            outs = eng.alloc_outputs(B, H, W)
            ws = eng.workspace(B, H, W)
            eng.forward_into(x, outs, in_layout, ws)
            if self.capture_visualization:
                self._capture(eng, ws, B, H, W)
            else:
                self.kfpn_features, self.fpn_outputs = [], {}
                self.kfpn_weights, self.backbone_features = {}, {}
        return outs

    def _capture(self, eng, ws, B, H, W):
        """Opt-in copies of the intermediate maps (fpn_resnet.py:189-242)."""
        views = eng.debug_views(ws, B, H, W)
        self.backbone_features = {k: views[k].clone() for k in ("layer1", "layer2", "layer3", "layer4")}
        self.kfpn_features = [views[k].clone() for k in ("up_level2", "up_level3", "up_level4")]
        self.fpn_outputs, self.kfpn_weights = {}, {}
        for name, lv in views["levels"].items():
            lv = [lv[0].repeat_interleave(2, 2).repeat_interleave(2, 3), lv[1], lv[2]]
            self.fpn_outputs[name] = [t.clone() for t in lv]
            self.kfpn_weights[name] = F.softmax(torch.stack(lv, dim=-1), dim=-1)

    def apply_kfpn(self, outs):
        """fpn_resnet.py:248-254 for one head: ``outs`` is a list of three equal-shaped (B, c, h, w) GPU tensors;
        returns (sum over the levels of v * softmax(v), the softmax weights (B, c, h, w, 3)).  One HIP launch
        (sfa_kfpn_combine), differentiable through sfa_kfpn_combine_grad; the weights carry no gradient (the
        reference only ever detaches them).  The model's own forward keeps its fused combine."""
        outs = list(outs)
        if len(outs) != 3:
            raise ValueError(f"apply_kfpn: {len(outs)} levels, expected 3")
        ret, weights = kfpn_heads({"head": outs}, level0_half=False, return_weights=True)
        return ret["head"], weights["head"]

    def get_visualization_data(self):
        return {"backbone_features": self.backbone_features, "kfpn_features": self.kfpn_features,
                "fpn_outputs": self.fpn_outputs, "kfpn_weights": self.kfpn_weights}

    def init_weights(self, num_layers, pretrained=True):
        if pretrained:
            raise RuntimeError("imagenet_pretrained=True downloads resnet weights "
                               "(fpn_resnet.py:283-286); no network access on this platform")


resnet_spec = {18: (BasicBlock, [2, 2, 2, 2])}


def get_pose_net(num_layers, heads, head_conv, imagenet_pretrained):
    if num_layers not in resnet_spec:
        raise NotImplementedError(f"fpn_resnet_{num_layers}: only 18 is implemented on gfx950")
    block_class, layers = resnet_spec[num_layers]
    model = PoseResNet(block_class, layers, heads, head_conv=head_conv)
    model.init_weights(num_layers, pretrained=imagenet_pretrained)
    return model


# names of the reference module this drop-in does not define come from the reference
__getattr__ = _dropin.module_getattr(__name__)
