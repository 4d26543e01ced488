"""FPN-ResNet-18 (KFPN) forward oracle in torch fp32 on CPU — TEST INFRASTRUCTURE ONLY.

A functional restatement of models/fpn_resnet.py that consumes a reference-format
state_dict (186 entries, names of fpn_resnet.py:114-151) and evaluates, in plain
torch CPU ops:

  stem           :120-123,179-182   conv7x7/s2/p3 -> BN(eps 1e-5) -> ReLU -> maxpool 3/2/1
  BasicBlock     :42-71             conv3x3(s)-BN-ReLU-conv3x3-BN (+downsample 1x1/s BN) + add, ReLU
  _make_layer    :153-167           resnet_spec[18] = [2, 2, 2, 2] (:289)
  FPN top-down   :197-210           bilinear x2 (align_corners=True) + cat + 1x1 conv (bias)
  heads          :133-145,219-233   per level & head: conv3x3(C->64, bias)-ReLU-conv1x1(64->c_h, bias);
                                    level 0 nearest-resized to H/4 x W/4
  apply_kfpn     :248-254           softmax over the 3 levels, sum(v * softmax(v))

It is both the numerics reference for the HIP conv path and the CPU baseline that
bench.py times on the GPU box's host cores (the reference Python cannot travel).

forward() is composed of stage functions (stage_layer1, stage_layer, stage_up, stage_heads,
stage_combine) that take whatever dtype their tensors have: with state_dict_torch(sd, torch.float64)
and f64 maps each one is the high-precision reference of one stage of the library's forward, on any
input (tests/stage_cases.py feeds them the GPU's own intermediate maps).
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

HEADS_DEFAULT = {"hm_cen": 3, "cen_offset": 2, "direction": 2, "z_coor": 1, "dim": 3}


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"],
                        sd[p + ".bias"], False, 0.0, 1e-5)


def _block(x, sd, p, stride):
    out = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"], None, stride, 1), sd, p + ".bn1"))
    out = _bn(F.conv2d(out, sd[p + ".conv2.weight"], None, 1, 1), sd, p + ".bn2")
    if p + ".downsample.0.weight" in sd:
        res = _bn(F.conv2d(x, sd[p + ".downsample.0.weight"], None, stride, 0), sd, p + ".downsample.1")
    else:
        res = x
    return F.relu(out + res)


def stage_layer1(sd: dict, x: torch.Tensor) -> torch.Tensor:
    """x (B, 3, H, W) -> layer1 (B, 64, H/4, W/4): stem conv, BN, ReLU, max-pool, layer1's two blocks."""
    y = F.relu(_bn(F.conv2d(x, sd["conv1.weight"], None, 2, 3), sd, "bn1"))
    y = F.max_pool2d(y, 3, 2, 1)
    y = _block(y, sd, "layer1.0", 1)
    return _block(y, sd, "layer1.1", 1)


def stage_layer(sd: dict, k: int, x: torch.Tensor) -> torch.Tensor:
    """layer(k-1) -> layer k for k = 2, 3, 4 (block 0 at stride 2 with its 1x1 downsample, block 1)."""
    y = _block(x, sd, f"layer{k}.0", 2)
    return _block(y, sd, f"layer{k}.1", 1)


def _up2(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


def stage_up(sd: dict, i: int, low: torch.Tensor, skip: torch.Tensor) -> torch.Tensor:
    """FPN level i = 0, 1, 2 -> the tensor the library keeps as up_level(i+2), the input of head level i:

      i = 0: low = layer4,    skip = layer3 -> up(conv_up_level1(cat(up(low), skip)))   (H/8,  256)
      i = 1: low = up_level2, skip = layer2 -> up(conv_up_level2(cat(low, skip)))       (H/4,  128)
      i = 2: low = up_level3, skip = layer1 -> conv_up_level3(cat(low, skip))           (H/4,   64)

    (fpn_resnet.py:197-210; `low` of levels 1 and 2 is already at the skip's resolution.)"""
    p = f"conv_up_level{i + 1}"
    if i == 0:
        low = _up2(low)
    c = F.conv2d(torch.cat((low, skip), 1), sd[p + ".weight"], sd[p + ".bias"])
    return _up2(c) if i < 2 else c


def stage_heads(sd: dict, level: int, inp: torch.Tensor, heads: dict = HEADS_DEFAULT) -> dict:
    """All heads of FPN level `level` on its input map: {head: (B, c, h, w)} at the level's own size."""
    out = {}
    for head in heads:
        p = f"fpn{level}_{head}"
        h = F.relu(F.conv2d(inp, sd[p + ".0.weight"], sd[p + ".0.bias"], 1, 1))
        out[head] = F.conv2d(h, sd[p + ".2.weight"], sd[p + ".2.bias"])
    return out


def stage_combine(levels, hm_h: int, hm_w: int, return_weights: bool = False):
    """apply_kfpn for one head: levels = its three per-level maps; a level of another size (level 0) is
    nearest-resized to (hm_h, hm_w), then softmax over the levels and the weighted sum."""
    lv = [F.interpolate(h, size=(hm_h, hm_w)) if h.shape[2] != hm_h or h.shape[3] != hm_w else h
          for h in levels]
    st = torch.stack(lv, dim=-1)
    w = F.softmax(st, dim=-1)
    out = (st * w).sum(dim=-1)
    return (out, w) if return_weights else out


def forward(sd: dict, x: torch.Tensor, heads: dict = HEADS_DEFAULT, return_viz: bool = False):
    """sd: reference state_dict of torch CPU tensors; x: (B, 3, H, W) of sd's dtype (f32, or f64 with
    state_dict_torch(sd, torch.float64))."""
    hm_h, hm_w = x.shape[2] // 4, x.shape[3] // 4
    l1 = stage_layer1(sd, x)
    l2 = stage_layer(sd, 2, l1)
    l3 = stage_layer(sd, 3, l2)
    l4 = stage_layer(sd, 4, l3)
    up2 = stage_up(sd, 0, l4, l3)
    up3 = stage_up(sd, 1, up2, l2)
    up4 = stage_up(sd, 2, up3, l1)
    lv = [stage_heads(sd, idx, inp, heads) for idx, inp in enumerate((up2, up3, up4))]
    ret, viz_w = {}, {}
    for head in heads:
        ret[head], viz_w[head] = stage_combine([lv[idx][head] for idx in range(3)], hm_h, hm_w, True)
    if return_viz:
        return ret, {"layer1": l1, "layer2": l2, "layer3": l3, "layer4": l4,
                     "kfpn": [up2, up3, up4], "kfpn_weights": viz_w}
    return ret


def state_dict_torch(sd_np: dict, dtype=torch.float32) -> dict:
    """numpy state_dict -> torch CPU tensors; floating entries as `dtype` (f64 for the high-precision
    reference), integer ones (num_batches_tracked) unchanged."""
    out = {}
    for k, v in sd_np.items():
        t = torch.from_numpy(v)
        out[k] = t.to(dtype) if t.is_floating_point() else t
    return out
