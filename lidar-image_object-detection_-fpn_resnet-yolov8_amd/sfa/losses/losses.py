"""Drop-in for the reference's losses/losses.py (:44-163): evaluation, and on request the gradient at
the five head maps.

``Compute_Loss(device).forward(outputs, tg)`` returns ``(total_loss, loss_stats)`` like the
reference — a 0-dim GPU tensor and the six-key dict — and leaves ``outputs['hm_cen']`` and
``outputs['cen_offset']`` holding the clamped sigmoid (:140-141).  Every term is evaluated by the HIP
library (sfa_compute_loss: float64 terms from the float32 operands, float64 sums in a fixed order,
rounded to float32 once).  By default nothing here is differentiable: a tensor with ``requires_grad``
raises NotImplementedError, CPU tensors are refused like in the rest of the drop-in.
``Compute_Loss(device, differentiable=True)`` makes ``total_loss.backward()`` work for the five logit
maps (sfa_compute_loss_grad); see the class.

``FocalLoss``, ``L1Loss``, ``L1Loss_Balanced`` and ``_neg_loss`` keep the reference's names and
signatures; each runs the same kernels with the other terms' inputs absent and returns its own
component as a 0-dim GPU tensor.
"""

from __future__ import annotations

import torch
import torch.nn as nn

from sfa_hip import dropin as _dropin
from sfa_hip import runtime as _rt
from utils.torch_utils import _sigmoid, to_cpu

_evaluators: dict = {}


def _evaluator(device) -> "_rt.LossEvaluator":
    key = str(device)
    ev = _evaluators.get(key)
    if ev is None:
        ev = _evaluators[key] = _rt.LossEvaluator(device)
    return ev


def _no_grad(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise NotImplementedError("losses (gfx950 drop-in): evaluation only — a tensor requires grad; "
                                      "detach it or run under torch.no_grad() (there is no backward pass)")


def _gpu(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _rt.SfaNativeError(f"{what}: the HIP path needs GPU tensors; there is no CPU fallback")
    return t


def _neg_loss(pred, gt, alpha=2, beta=4):
    """Modified focal loss (:44-69) of clamped probabilities ``pred`` against ``gt``, both (B, C, H, W)."""
    if alpha != 2 or beta != 4:
        raise NotImplementedError("_neg_loss: the kernel evaluates alpha = 2, beta = 4 (the reference's only use)")
    _no_grad(pred, gt)
    pred, gt = _gpu(pred, "_neg_loss"), _gpu(gt, "_neg_loss")
    B, C, H, W = (int(v) for v in pred.shape)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=pred.device)  # noqa: E731
    outs = {"hm_cen": pred, "cen_offset": z(B, 2, H, W), "direction": z(B, 2, H, W), "z_coor": z(B, 1, H, W),
            "dim": z(B, 3, H, W)}
    tg = {"hm_cen": gt, "cen_offset": z(B, 1, 2), "direction": z(B, 1, 2), "z_coor": z(B, 1, 1), "dim": z(B, 1, 3),
          "indices_center": z(B, 1, dt=torch.int64), "obj_mask": z(B, 1, dt=torch.uint8)}
    return _evaluator(pred.device)(outs, tg)[1].clone()


class FocalLoss(nn.Module):
    """nn.Module wrapper for the focal loss (:72-80)."""

    def __init__(self):
        super().__init__()
        self.neg_loss = _neg_loss

    def forward(self, out, target):
        return self.neg_loss(out, target)


def _masked(output, mask, ind, target, slot, component):
    """One masked L1 term through sfa_compute_loss: ``output`` (B, c, H, W) stands in the head of ``slot``
    (whose channel count is c); the other heads are zeros against zero targets, so their sums stay zero
    and ``component`` of the result is this term alone."""
    _no_grad(output, target)
    output, target = _gpu(output, "L1Loss"), _gpu(target, "L1Loss")
    B, c, H, W = (int(v) for v in output.shape)
    M = int(ind.shape[1])
    if c != _rt.DEFAULT_HEADS[slot]:
        raise NotImplementedError(f"L1Loss: {c} channels; the kernels cover the reference's heads "
                                  f"(cen_offset / direction 2, z_coor 1, dim 3)")
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=output.device)  # noqa: E731
    outs = {k: z(B, ch, H, W) for k, ch in _rt.DEFAULT_HEADS.items()}
    outs["hm_cen"] = torch.full((B, 1, H, W), 0.5, dtype=torch.float32, device=output.device)
    tg = {"hm_cen": z(B, 1, H, W), "cen_offset": z(B, M, 2), "direction": z(B, M, 2), "z_coor": z(B, M, 1),
          "dim": z(B, M, 3), "indices_center": ind, "obj_mask": mask}
    outs[slot], tg[slot] = output, target
    return _evaluator(output.device)(outs, tg)[component].clone()


class L1Loss(nn.Module):
    """Masked L1 (:83-92) of a 2-channel head: sum |pred*m - t*m| / (m.sum() + 1e-4)."""

    def forward(self, output, mask, ind, target):
        return _masked(output, mask, ind, target, "direction", 4)


class L1Loss_Balanced(nn.Module):
    """Balanced L1 (:95-125) of z_coor (1 channel) or dim (3 channels), alpha 0.5, gamma 1.5, beta 1."""

    def __init__(self, alpha=0.5, gamma=1.5, beta=1.0):
        super().__init__()
        if (alpha, gamma, beta) != (0.5, 1.5, 1.0):
            raise NotImplementedError("L1Loss_Balanced: the kernel evaluates alpha 0.5, gamma 1.5, beta 1.0")
        self.alpha, self.gamma, self.beta = alpha, gamma, beta

    def forward(self, output, mask, ind, target):
        one = int(output.shape[1]) == 1
        return _masked(output, mask, ind, target, "z_coor" if one else "dim", 5 if one else 3)


class _LossAtHeads(torch.autograd.Function):
    """total_loss of the five logit maps with its gradient at those maps, both from the HIP library.
    forward evaluates the loss on the raw logits (apply_sigmoid = 1) and, when a map requires grad,
    sfa_compute_loss_grad; the five gradient maps are what is saved (never the logits, which the caller
    may overwrite).  backward scales them by the upstream scalar."""

    @staticmethod
    def forward(ctx, evaluator, tg, *logits):
        outs = dict(zip(_rt.DEFAULT_HEADS, logits))
        stats = evaluator(outs, tg, apply_sigmoid=True).clone()
        ctx.have = any(ctx.needs_input_grad[2:])
        if ctx.have:
            grads = evaluator.grad(outs, tg, apply_sigmoid=True)
            ctx.save_for_backward(*(grads[k] for k in _rt.DEFAULT_HEADS))
        ctx.mark_non_differentiable(stats)
        return stats[0].clone(), stats

    @staticmethod
    def backward(ctx, upstream, _stats):
        if not ctx.have:
            return (None,) * 7
        return (None, None) + tuple(g * upstream if need else None
                                    for g, need in zip(ctx.saved_tensors, ctx.needs_input_grad[2:]))


class Compute_Loss(nn.Module):
    """The reference's Compute_Loss (:128-163).  ``differentiable=False`` (the default) is evaluation
    only.  With ``differentiable=True`` ``total_loss`` carries a grad_fn and ``total_loss.backward()``
    leaves d total / d logits at the five head maps (sfa_compute_loss_grad; unit weights only); nothing
    behind the head maps is part of this module.  Departure from :140-141 in that mode:
    ``outputs['hm_cen']`` and ``outputs['cen_offset']`` still hold the clamped sigmoid afterwards, but as
    new, detached tensors (the logits are left untouched for autograd), so a later use of those two
    entries does not back-propagate."""

    def __init__(self, device, differentiable=False):
        super().__init__()
        self.device = device
        self.differentiable = bool(differentiable)
        self.focal_loss = FocalLoss()
        self.l1_loss = L1Loss()
        self.l1_loss_balanced = L1Loss_Balanced(alpha=0.5, gamma=1.5, beta=1.0)
        self.weight_hm_cen = 1.
        self.weight_z_coor, self.weight_cenoff, self.weight_dim, self.weight_direction = 1., 1., 1., 1.

    def forward(self, outputs, tg):
        if self.differentiable:
            _no_grad(*tg.values())
        else:
            _no_grad(*outputs.values(), *tg.values())
        for k in _rt.DEFAULT_HEADS:
            _gpu(outputs[k], f"Compute_Loss outputs[{k!r}]")
        weights = (self.weight_hm_cen, self.weight_cenoff, self.weight_dim, self.weight_direction, self.weight_z_coor)
        if any(w != 1. for w in weights):
            raise NotImplementedError("Compute_Loss: the kernel sums the terms with the reference's unit weights")
        if self.differentiable:
            logits = [outputs[k] for k in _rt.DEFAULT_HEADS]
            total, loss = _LossAtHeads.apply(_evaluator(logits[0].device), tg, *logits)
            for k in ('hm_cen', 'cen_offset'):
                outputs[k] = _sigmoid(outputs[k].detach().clone(memory_format=torch.contiguous_format))
            host = to_cpu(loss).tolist()
            return total, dict(zip(_rt.LOSS_KEYS, host))
        outputs['hm_cen'] = _sigmoid(outputs['hm_cen'])
        outputs['cen_offset'] = _sigmoid(outputs['cen_offset'])
        loss = _evaluator(outputs['hm_cen'].device)(outputs, tg).clone()
        host = to_cpu(loss).tolist()
        return loss[0], dict(zip(_rt.LOSS_KEYS, host))


# names of the reference module this drop-in does not define come from the reference
__getattr__ = _dropin.module_getattr(__name__)
