"""ResNet-50 (torchvision v1.5 topology) -- BASELINE.json config "ResNet-50-sized CNN DDP 8x" --
and ResNeXt-50 32x4d, the same network with a grouped 3x3 (``Bottleneck(groups=, base_width=)``,
csrc/conv_grouped.hip).

``state_dict`` keys match ``torchvision.models.resnet50`` (conv1/bn1/layer1-4/fc, Bottleneck
conv1-3/bn1-3/downsample.{0,1}); stride sits on the 3x3 conv (v1.5). 25.6 M parameters in 161
tensors -- many small gradients, which is what stresses the bucketed all-reduce overlap (SURVEY.md
§2.6). ReLU is fused into the batch-norm kernels (``relu=True``) and the residual join
``relu(bn3(conv3) + identity)`` is fused into bn3's normalisation pass (and its backward). ``convert_sync_batchnorm`` turns the BatchNorm2d layers into SyncBatchNorm.
Weights use torchvision's initialisation (Kaiming-normal fan_out convs, BN gamma=1 beta=0).

``norm_layer`` (``Bottleneck`` and ``ResNet``) swaps the normalisation: a callable
``(channels, relu=False, device=None) -> module``; the default builds today's ``BatchNorm2d``.
``resnet50_gn`` uses ``GroupNorm(32, channels)`` (csrc/groupnorm.hip) -- the network
``torchvision.models.resnet50(norm_layer=lambda c: nn.GroupNorm(32, c))`` builds, with the same
attribute names (``bn1`` ...), no buffers, and no batch statistics asked of the convolutions.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..ops._grad import SharedGrad, fork
from ..nn import AdaptiveAvgPool2d, BatchNorm2d, Conv2d, GroupNorm, Linear, MaxPool2d


def _batch_norm(channels, relu=False, device=None):
    return BatchNorm2d(channels, relu=relu, device=device)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, device=None, groups=1,
                 base_width=64, norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or _batch_norm
        kw = dict(bias=False, device=device)
        # torchvision's width rule: ResNeXt widens the 3x3 and splits it into groups
        width = int(planes * base_width / 64) * groups
        self.conv1 = Conv2d(inplanes, width, 1, **kw)
        self.bn1 = norm_layer(width, relu=True, device=device)
        self.conv2 = Conv2d(width, width, 3, stride=stride, padding=1, groups=groups, **kw)
        self.bn2 = norm_layer(width, relu=True, device=device)
        self.conv3 = Conv2d(width, planes * 4, 1, **kw)
        self.bn3 = norm_layer(planes * 4, device=device)
        self.downsample = downsample
        self.stride = stride
        self._fused_join = True

    def forward(self, x):
        if self._fused_join and hasattr(self.bn3, "relu_join"):
            return self._forward_fused(x)
        out = self.bn1(self.conv1(x))
        out = self.bn2(self.conv2(out))
        identity = self.downsample(x) if self.downsample is not None else x
        out = self.bn3(self.conv3(out))
        return ops.add_relu(out, identity)

    def _forward_fused(self, x):
        # relu(bn3(conv3(.)) + identity) in the normalisation pass; its backward writes the
        # identity gradient in the same pass as bn3's (no separate add/ReLU-mask kernels).
        # x's two consumers (conv1, identity path) share ONE gradient buffer (ops/_grad.py
        # SharedGrad): bn3's backward (or the downsample conv's input gradient) writes it and
        # conv1's input-gradient GEMM accumulates into it -- no autograd add of the two.
        sink = None
        xa = xb = x
        if torch.is_grad_enabled() and x.requires_grad:
            sink = SharedGrad()
            xa, xb = fork(x, sink)
        out = self.bn1(self.conv1(xa, grad_into=sink) if _takes_sink(self.conv1) else
                       self.conv1(xa))
        out = self.bn2(self.conv2(out))
        ds = self.downsample
        if ds is None:
            return self.bn3.relu_join(self.conv3(out), xb, grad_into=sink)
        if isinstance(ds, nn.Sequential) and len(ds) == 2 and _takes_sink(ds[0]):
            identity = ds[1](ds[0](xb, grad_into=sink))
        else:
            identity = ds(xb)
        return self.bn3.relu_join(self.conv3(out), identity)


def _takes_sink(m) -> bool:
    return isinstance(m, Conv2d)


class ResNet(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), num_classes: int = 10, device=None, groups=1,
                 width_per_group=64, norm_layer=None):
        super().__init__()
        self._norm_layer = norm_layer or _batch_norm
        self.inplanes = 64
        self.groups, self.base_width = groups, width_per_group
        self.conv1 = Conv2d(3, 64, 7, stride=2, padding=3, bias=False, device=device)
        self.bn1 = self._norm_layer(64, relu=True, device=device)
        self.maxpool = MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0], 1, device)
        self.layer2 = self._make_layer(128, layers[1], 2, device)
        self.layer3 = self._make_layer(256, layers[2], 2, device)
        self.layer4 = self._make_layer(512, layers[3], 2, device)
        self.avgpool = AdaptiveAvgPool2d((1, 1))
        self.fc = Linear(512 * Bottleneck.expansion, num_classes, device=device)
        # every convolution here feeds a BatchNorm: its GEMM epilogue emits the statistics
        # (per-channel batch statistics are of no use to another normalisation)
        for conv, norm in self._conv_norm_pairs():
            if isinstance(norm, nn.modules.batchnorm._BatchNorm):
                conv.bn_stats = True
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        del self._norm_layer  # construction only (a closure would not pickle with the model)

    def _conv_norm_pairs(self):
        yield self.conv1, self.bn1
        for m in self.modules():
            if isinstance(m, Bottleneck):
                yield m.conv1, m.bn1
                yield m.conv2, m.bn2
                yield m.conv3, m.bn3
                if m.downsample is not None and isinstance(m.downsample[0], Conv2d):
                    yield m.downsample[0], m.downsample[1]

    def _make_layer(self, planes, blocks, stride, device):
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(
                Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False, device=device),
                self._norm_layer(planes * 4, device=device))
        kw = dict(device=device, groups=self.groups, base_width=self.base_width,
                  norm_layer=self._norm_layer)
        layers = [Bottleneck(self.inplanes, planes, stride, downsample, **kw)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.inplanes, planes, **kw))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.bn1(self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.avgpool(x)
        return self.fc(x.reshape(x.shape[0], -1))


def resnet50(num_classes: int = 10, device=None) -> ResNet:
    return ResNet((3, 4, 6, 3), num_classes=num_classes, device=device)


def resnext50_32x4d(num_classes: int = 10, device=None) -> ResNet:
    """ResNeXt-50 32x4d (torchvision topology and state_dict keys): ResNet-50's block with a
    32-group 3x3 of 4 channels per group at layer1, doubling per stage."""
    return ResNet((3, 4, 6, 3), num_classes=num_classes, device=device, groups=32,
                  width_per_group=4)


def resnet50_gn(num_classes: int = 10, device=None, groups: int = 32) -> ResNet:
    """ResNet-50 with ``GroupNorm(groups, channels)`` in place of every BatchNorm (weight 1,
    bias 0, no buffers): per-sample statistics, so no SyncBatchNorm conversion is needed under
    data parallelism."""
    def norm(channels, relu=False, device=None):
        return GroupNorm(groups, channels, relu=relu, device=device)

    return ResNet((3, 4, 6, 3), num_classes=num_classes, device=device, norm_layer=norm)
