"""Drop-in for the reference's models/resnet.py — the plain CenterNet-style ResNet on gfx950.

The module tree mirrors the reference's registration order exactly (resnet.py:117-158: stem, layer1-4,
``deconv_layers`` = three ConvTranspose2d(4, stride 2, pad 1, bias=False) + BatchNorm + ReLU, then the
heads in sorted() order under their plain names), so ``load_state_dict(strict=True)`` accepts the
reference's ``resnet_18`` checkpoints and ``state_dict()`` round-trips them.  The submodules are
parameter containers only: ``PoseResNet.forward`` packs them (BatchNorm folded; each transposed conv as
the four 2 x 2 phase matrices of its output parities) into one device buffer on first use / after any
parameter change, and runs the whole forward — stem, 8 BasicBlocks, the three transposed convs, the
fused heads — as HIP kernels (libsfa_hip.so, SFA_BACKBONE_DECONV).  There is no CPU path: a CPU input
raises ``SfaNativeError``.  The arithmetic is fp16x3 (``set_math`` of any other mode raises: the
transposed convolutions have no other kernel).  Like the reference's file, no visualisation capture.
"""

from __future__ import annotations

import torch
import torch.nn as nn

from models import fpn_resnet as _fpn
from models.fpn_resnet import BN_MOMENTUM, BasicBlock, conv3x3, model_urls  # noqa: F401
from sfa_hip import _lib
from sfa_hip import dropin as _dropin


class PoseResNet(_fpn.PoseResNet):
    """resnet.py:115-234.  The engine plumbing (weight repacking on change, per-device engines,
    ``set_math``) is fpn_resnet.PoseResNet's; the module tree and the forward are this family's."""

    def __init__(self, block, layers, heads, head_conv, **kwargs):
        self.inplanes = 64
        self.deconv_with_bias = False
        self.heads = heads
        nn.Module.__init__(self)
        if block is not BasicBlock or list(layers) != [2, 2, 2, 2]:
            raise NotImplementedError("the HIP forward implements resnet_18 (BasicBlock x [2,2,2,2])")
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
        self.deconv_layers = self._make_deconv_layer(3, [256, 256, 256], [4, 4, 4])
        for head in sorted(self.heads):
            self.__setattr__(head, nn.Sequential(
                nn.Conv2d(256, head_conv, kernel_size=3, padding=1, bias=True),
                nn.ReLU(inplace=True),
                nn.Conv2d(head_conv, self.heads[head], kernel_size=1, stride=1, padding=0)))
        self._arch = _lib.make_arch(dict(self.heads), head_conv, backbone=_lib.BACKBONE_DECONV)
        self._engines = {}
        self._math = None
        self._sig = None
        self._state_tensors = None

    def _get_deconv_cfg(self, deconv_kernel, index):
        if deconv_kernel != 4:
            raise NotImplementedError("the HIP forward implements 4 x 4 / stride 2 / pad 1 transposed convs")
        return deconv_kernel, 1, 0

    def _make_deconv_layer(self, num_layers, num_filters, num_kernels):
        assert num_layers == len(num_filters), "ERROR: num_deconv_layers is different len(num_deconv_filters)"
        assert num_layers == len(num_kernels), "ERROR: num_deconv_layers is different len(num_deconv_filters)"
        layers = []
        for i in range(num_layers):
            kernel, padding, output_padding = self._get_deconv_cfg(num_kernels[i], i)
            planes = num_filters[i]
            layers.append(nn.ConvTranspose2d(in_channels=self.inplanes, out_channels=planes, kernel_size=kernel,
                                             stride=2, padding=padding, output_padding=output_padding,
                                             bias=self.deconv_with_bias))
            layers.append(nn.BatchNorm2d(planes, momentum=BN_MOMENTUM))
            layers.append(nn.ReLU(inplace=True))
            self.inplanes = planes
        return nn.Sequential(*layers)

    def forward(self, x):
        return self.forward_layout(x, _lib.IN_NCHW3)

    def forward_layout(self, x, in_layout):
        """The heads dict in insertion order (resnet.py:231-234); ``in_layout`` as fpn_resnet's."""
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
            raise _lib.SfaNativeError("PoseResNet.forward runs on the GPU (HIP) only; move the "
                                      "model input to a GPU device")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected (B, 3, H, W), got {tuple(x.shape)}")
        if in_layout not in (_lib.IN_NCHW3, _lib.IN_NCHW3_FLIP_HW):
            raise ValueError(f"unsupported input layout {in_layout}")
        eng = self._engine(x.device)
        x = x.contiguous().float()
        with torch.no_grad(), torch.cuda.device(x.device):
            B, _, H, W = x.shape
            outs = eng.alloc_outputs(B, H, W)
            eng.forward_into(x, outs, in_layout, eng.workspace(B, H, W))
        return outs

    def apply_kfpn(self, outs):
        raise AttributeError("the plain resnet has no KFPN (models/resnet.py)")

    def get_visualization_data(self):
        raise AttributeError("the plain resnet captures no visualisation data (models/resnet.py)")


resnet_spec = {18: (BasicBlock, [2, 2, 2, 2])}


def get_pose_net(num_layers, heads, head_conv, imagenet_pretrained):
    if num_layers not in resnet_spec:
        raise NotImplementedError(f"resnet_{num_layers}: only 18 is implemented on gfx950")
    block_class, layers = resnet_spec[num_layers]
    model = PoseResNet(block_class, layers, heads, head_conv=head_conv)
    model.init_weights(num_layers, pretrained=imagenet_pretrained)
    return model


# names of the reference module this drop-in does not define come from the reference
__getattr__ = _dropin.module_getattr(__name__)
