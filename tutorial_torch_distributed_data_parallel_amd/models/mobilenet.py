"""MobileNetV2 (torchvision topology): the network built on the depthwise kernels of
csrc/conv_grouped.hip.

``state_dict`` keys match ``torchvision.models.mobilenet_v2``: ``features.0.{0,1}`` (stem),
``features.N.conv.{0.0, 0.1, 1.0, 1.1, 2, 3}`` for an expansion block (1x1 expand + BN, depthwise
3x3 + BN, 1x1 project, BN) and ``features.1.conv.{0.0, 0.1, 1, 2}`` for the ``t = 1`` block,
``features.18.{0,1}`` (last 1x1) and ``classifier.1``. 3.5 M parameters in 158 tensors at 1000
classes. A conv-BN-ReLU6 triple is ``Sequential(Conv2d, BatchNorm2d(relu6=True))``: the ReLU6 --
the network's only activation -- runs inside the BatchNorm kernels and has no parameters, so the
keys are torchvision's ``Conv2dNormActivation`` keys. The linear-bottleneck residual
``x + bn(conv(.))`` (no activation) is the fused residual join of the last BatchNorm's
normalisation pass, and the block input's two consumers share one gradient buffer, as in
``models/resnet.py``. ``_make_divisible(., 8)`` is torchvision's width rule: every channel count
at width 1.0 and 0.75 is a multiple of 8, which the dense and the depthwise kernels take.
Weights use torchvision's initialisation (Kaiming-normal fan_out convolutions, BN 1 / 0, Linear
N(0, 0.01) with zero bias).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..nn import BatchNorm2d, Conv2d, Dropout, Linear
from ..ops import adaptive_avg_pool2d
from ..ops._grad import SharedGrad, fork


def _make_divisible(v: float, divisor: int = 8, min_value: int | None = None) -> int:
    """Round ``v`` to the nearest multiple of ``divisor`` without losing more than 10 %."""
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _conv_bn(cin, cout, kernel, stride=1, groups=1, relu6=True, device=None):
    """Conv2d (no bias, feeding the BatchNorm its statistics) + BatchNorm2d with a fused ReLU6."""
    conv = Conv2d(cin, cout, kernel, stride=stride, padding=(kernel - 1) // 2, groups=groups,
                  bias=False, device=device)
    conv.bn_stats = True
    return conv, BatchNorm2d(cout, relu6=relu6, device=device)


class InvertedResidual(nn.Module):
    """1x1 expand (``t`` > 1) -> depthwise 3x3 -> linear 1x1 project; ``x +`` when the block
    keeps the shape (stride 1, in = out)."""

    def __init__(self, inp: int, oup: int, stride: int, t: int, device=None):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError(f"InvertedResidual: stride must be 1 or 2, got {stride}")
        hidden = int(round(inp * t))
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if t != 1:
            layers.append(nn.Sequential(*_conv_bn(inp, hidden, 1, device=device)))
        layers.append(nn.Sequential(*_conv_bn(hidden, hidden, 3, stride=stride, groups=hidden,
                                              device=device)))
        layers.extend(_conv_bn(hidden, oup, 1, relu6=False, device=device))
        self.conv = nn.Sequential(*layers)
        self._fused_join = True

    def forward(self, x):
        if not self.use_res_connect:
            return self.conv(x)
        if not self._fused_join:
            return x + self.conv(x)
        # x + bn(conv(.)) in the last normalisation pass; x's two consumers (the first
        # convolution, the identity) share ONE gradient buffer (ops/_grad.py SharedGrad): the
        # BatchNorm backward writes it and the first convolution's input gradient accumulates
        sink = None
        xa = xb = x
        if torch.is_grad_enabled() and x.requires_grad:
            sink = SharedGrad()
            xa, xb = fork(x, sink)
        first = self.conv[0]  # a (Conv2d, BatchNorm2d) pair for every t
        out = first[1](first[0](xa, grad_into=sink))
        for m in list(self.conv)[1:-1]:
            out = m(out)
        return self.conv[-1](out, residual=xb, relu=False, residual_grad_into=sink)


class MobileNetV2(nn.Module):
    # (expansion t, output channels c, repeats n, first stride s)
    SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1),
               (6, 160, 3, 2), (6, 320, 1, 1))

    def __init__(self, num_classes: int = 10, width_mult: float = 1.0, device=None,
                 dropout: float = 0.2):
        super().__init__()
        inp = _make_divisible(32 * width_mult)
        self.last_channel = _make_divisible(1280 * max(1.0, width_mult))
        features = [nn.Sequential(*_conv_bn(3, inp, 3, stride=2, device=device))]
        for t, c, n, s in self.SETTING:
            oup = _make_divisible(c * width_mult)
            for i in range(n):
                features.append(InvertedResidual(inp, oup, s if i == 0 else 1, t, device=device))
                inp = oup
        features.append(nn.Sequential(*_conv_bn(inp, self.last_channel, 1, device=device)))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(Dropout(dropout),
                                        Linear(self.last_channel, num_classes, device=device))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
            elif isinstance(m, nn.modules.batchnorm._BatchNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.features(x)
        x = adaptive_avg_pool2d(x, (1, 1))
        return self.classifier(x.reshape(x.shape[0], -1))


def mobilenet_v2(num_classes: int = 10, width_mult: float = 1.0, device=None) -> MobileNetV2:
    return MobileNetV2(num_classes=num_classes, width_mult=width_mult, device=device)
