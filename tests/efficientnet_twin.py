"""EfficientNet-B0 in plain torch.nn, module for module torchvision's ``efficientnet_b0`` (same
``state_dict`` keys: the SiLU of a conv-BN-SiLU triple sits at index 2 and has no parameters):
the twin the EfficientNet tests compare ``models/efficientnet.py`` against, so a ``state_dict`` of
either loads into the other. 5,288,548 parameters at 1000 classes (torchvision's figure)."""
import torch
import torch.nn as nn

from mobilenet_twin import U, check_grads_rule, check_rule, grad_scales  # noqa: F401

# (expand, kernel, stride, in, out, repeats)
SETTING = ((1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3),
           (6, 5, 1, 80, 112, 3), (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1))


def conv_bn_act(cin, cout, kernel=3, stride=1, groups=1, act=True):
    layers = [nn.Conv2d(cin, cout, kernel, stride, (kernel - 1) // 2, groups=groups, bias=False),
              nn.BatchNorm2d(cout)]
    if act:
        layers.append(nn.SiLU())
    return nn.Sequential(*layers)


class TwinSqueezeExcitation(nn.Module):
    def __init__(self, input_channels, squeeze_channels):
        super().__init__()
        self.fc1 = nn.Conv2d(input_channels, squeeze_channels, 1)
        self.fc2 = nn.Conv2d(squeeze_channels, input_channels, 1)

    def forward(self, x):
        s = nn.functional.adaptive_avg_pool2d(x, 1)
        s = self.fc2(nn.functional.silu(self.fc1(s)))
        return x * torch.sigmoid(s)


class TwinStochasticDepth(nn.Module):
    """Row mode, torchvision's arithmetic."""

    def __init__(self, p):
        super().__init__()
        self.p = p

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        keep = 1.0 - self.p
        noise = torch.empty([x.shape[0]] + [1] * (x.dim() - 1), dtype=x.dtype, device=x.device)
        noise.bernoulli_(keep)
        if keep > 0.0:
            noise.div_(keep)
        return x * noise


class TwinMBConv(nn.Module):
    def __init__(self, inp, oup, stride, kernel, expand, sd_prob=0.0):
        super().__init__()
        hidden = inp * expand
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if expand != 1:
            layers.append(conv_bn_act(inp, hidden, 1))
        layers += [conv_bn_act(hidden, hidden, kernel, stride, groups=hidden),
                   TwinSqueezeExcitation(hidden, max(1, inp // 4)),
                   conv_bn_act(hidden, oup, 1, act=False)]
        self.block = nn.Sequential(*layers)
        self.stochastic_depth = TwinStochasticDepth(sd_prob)

    def forward(self, x):
        y = self.block(x)
        return x + self.stochastic_depth(y) if self.use_res_connect else y


class TwinEfficientNetB0(nn.Module):
    def __init__(self, num_classes=10, stochastic_depth_prob=0.2, dropout=0.2):
        super().__init__()
        total = sum(s[5] for s in SETTING)
        features = [conv_bn_act(3, 32, 3, 2)]
        b = 0
        for expand, kernel, stride, inp, oup, repeats in SETTING:
            stage = []
            for i in range(repeats):
                stage.append(TwinMBConv(inp if i == 0 else oup, oup, stride if i == 0 else 1,
                                        kernel, expand, stochastic_depth_prob * b / total))
                b += 1
            features.append(nn.Sequential(*stage))
        features.append(conv_bn_act(320, 1280, 1))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(nn.Dropout(dropout), nn.Linear(1280, num_classes))

    def forward(self, x):
        x = self.features(x)
        x = nn.functional.adaptive_avg_pool2d(x, (1, 1))
        return self.classifier(x.flatten(1))
