"""EfficientNet-B0 (torchvision topology): MobileNetV2's inverted-residual skeleton with SiLU,
squeeze-and-excitation and stochastic depth. CPU tensors only so far: SiLU (stand-alone and in
BatchNorm) and the squeeze-excitation gate have no gfx950 kernels yet, so a forward on a GPU
tensor raises at the first BatchNorm (profiles/r19/efficientnet_b0.md).

``state_dict`` keys match ``torchvision.models.efficientnet_b0``: ``features.0.{0,1}`` (stem,
3 -> 32, 3x3, stride 2), ``features.S.I.block.J`` for block I of stage S = 1..7 -- ``block.0``
1x1 expand + BN (omitted when the expansion is 1), then depthwise k x k + BN, the
``SqueezeExcitation`` (``fc1`` / ``fc2``, 1x1 convolutions WITH bias, squeeze width
``max(1, block_in // 4)``) and the linear 1x1 project + BN, each conv-BN a ``{0, 1}`` pair --
``features.8.{0,1}`` (head, 320 -> 1280) and ``classifier.1``. 5,288,548 parameters at 1000
classes. A conv-BN-SiLU triple is ``Sequential(Conv2d(bias=False, bn_stats=True),
BatchNorm2d(silu=True))``: the SiLU is the BatchNorm op's activation kind 3 and has
no parameters, so the keys are torchvision's ``Conv2dNormActivation`` keys, and the depthwise
layers keep their statistics epilogue. Block b of the 16 drops its residual branch per sample
with probability ``stochastic_depth_prob * b / 16``. The residual join (stride 1, in = out) is
the fused BatchNorm residual join with one shared gradient buffer for the block input's two
consumers, exactly as ``models/mobilenet.py``, whenever the branch is not dropped (probability 0,
or eval); in training with a probability > 0 it runs unfused, ``x + stochastic_depth(.)``.
Weights use torchvision's initialisation: Kaiming-normal fan_out convolutions (zero bias), BN
1 / 0, Linear uniform +-1/sqrt(out_features) with zero bias; BN eps and momentum are torch's
defaults.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from ..nn import BatchNorm2d, Conv2d, Dropout, Linear, SqueezeExcitation, StochasticDepth
from ..ops import adaptive_avg_pool2d
from ..ops._grad import SharedGrad, fork


def _conv_bn(cin, cout, kernel, stride=1, groups=1, silu=True, device=None):
    """Conv2d (no bias, feeding the BatchNorm its statistics) + BatchNorm2d with a fused SiLU."""
    conv = Conv2d(cin, cout, kernel, stride=stride, padding=(kernel - 1) // 2, groups=groups,
                  bias=False, device=device)
    conv.bn_stats = True
    return nn.Sequential(conv, BatchNorm2d(cout, silu=silu, device=device))


class MBConv(nn.Module):
    """1x1 expand (``expand`` > 1) -> depthwise k x k -> squeeze-excitation -> linear 1x1
    project; ``x + stochastic_depth(.)`` when the block keeps the shape (stride 1, in = out)."""

    def __init__(self, inp: int, oup: int, stride: int, kernel: int, expand: int,
                 sd_prob: float = 0.0, device=None):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError(f"MBConv: stride must be 1 or 2, got {stride}")
        hidden = inp * expand
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if expand != 1:
            layers.append(_conv_bn(inp, hidden, 1, device=device))
        layers.append(_conv_bn(hidden, hidden, kernel, stride=stride, groups=hidden,
                               device=device))
        layers.append(SqueezeExcitation(hidden, max(1, inp // 4), device=device))
        layers.append(_conv_bn(hidden, oup, 1, silu=False, device=device))
        self.block = nn.Sequential(*layers)
        self.stochastic_depth = StochasticDepth(sd_prob, "row")
        self._fused_join = True

    def forward(self, x):
        if not self.use_res_connect:
            return self.block(x)
        if (self.training and self.stochastic_depth.p > 0) or not self._fused_join:
            return x + self.stochastic_depth(self.block(x))
        # x + bn(conv(.)) in the last normalisation pass; x's two consumers (the first
        # convolution, the identity) share ONE gradient buffer (ops/_grad.py SharedGrad), as in
        # models/mobilenet.py
        sink = None
        xa = xb = x
        if torch.is_grad_enabled() and x.requires_grad:
            sink = SharedGrad()
            xa, xb = fork(x, sink)
        first, last = self.block[0], self.block[-1]
        out = first[1](first[0](xa, grad_into=sink))
        for m in list(self.block)[1:-1]:
            out = m(out)
        return last[1](last[0](out), residual=xb, relu=False, residual_grad_into=sink)


class EfficientNet(nn.Module):
    # (expand, kernel, stride, in, out, repeats): EfficientNet-B0 (width and depth 1.0)
    SETTING = ((1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2),
               (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3), (6, 5, 2, 112, 192, 4),
               (6, 3, 1, 192, 320, 1))

    def __init__(self, num_classes: int = 10, device=None, stochastic_depth_prob: float = 0.2,
                 dropout: float = 0.2):
        super().__init__()
        total = sum(s[5] for s in self.SETTING)
        features = [_conv_bn(3, self.SETTING[0][3], 3, stride=2, device=device)]
        b = 0
        for expand, kernel, stride, inp, oup, repeats in self.SETTING:
            stage = []
            for i in range(repeats):
                stage.append(MBConv(inp if i == 0 else oup, oup, stride if i == 0 else 1, kernel,
                                    expand, stochastic_depth_prob * b / total, device=device))
                b += 1
            features.append(nn.Sequential(*stage))
        last_in = self.SETTING[-1][4]
        self.last_channel = 4 * last_in
        features.append(_conv_bn(last_in, self.last_channel, 1, device=device))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(Dropout(dropout),
                                        Linear(self.last_channel, num_classes, device=device))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.modules.batchnorm._BatchNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                r = 1.0 / math.sqrt(m.out_features)
                nn.init.uniform_(m.weight, -r, r)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.features(x)
        x = adaptive_avg_pool2d(x, (1, 1))
        return self.classifier(x.reshape(x.shape[0], -1))


def efficientnet_b0(num_classes: int = 10, device=None, stochastic_depth_prob: float = 0.2,
                    dropout: float = 0.2) -> EfficientNet:
    return EfficientNet(num_classes=num_classes, device=device,
                        stochastic_depth_prob=stochastic_depth_prob, dropout=dropout)
