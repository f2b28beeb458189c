"""A plain ``torch.nn`` ResNet-50 with GroupNorm, written by hand after torchvision's
``resnet50(norm_layer=lambda c: nn.GroupNorm(groups, c))`` (v1.5: the stride sits on the 3x3), as
the oracle of the GroupNorm tests, and a small Conv-Norm-Linear net for the DDP property."""
import torch
import torch.nn as nn


class TwinBottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample, groups):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.GroupNorm(groups, planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.GroupNorm(groups, planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.GroupNorm(groups, planes * 4)
        self.relu = nn.ReLU()
        self.downsample = downsample

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return self.relu(out + identity)


class TwinResNetGN(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), num_classes=10, groups=32):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.GroupNorm(groups, 64)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make(64, layers[0], 1, groups)
        self.layer2 = self._make(128, layers[1], 2, groups)
        self.layer3 = self._make(256, layers[2], 2, groups)
        self.layer4 = self._make(512, layers[3], 2, groups)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(2048, num_classes)

    def _make(self, planes, blocks, stride, groups):
        ds = None
        if stride != 1 or self.inplanes != planes * 4:
            ds = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False),
                               nn.GroupNorm(groups, planes * 4))
        out = [TwinBottleneck(self.inplanes, planes, stride, ds, groups)]
        self.inplanes = planes * 4
        out += [TwinBottleneck(self.inplanes, planes, 1, None, groups) for _ in range(1, blocks)]
        return nn.Sequential(*out)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def small_net(norm: str, tdp_nn=None):
    """Conv(3->8) - norm - ReLU - pool - Linear(8->4); ``norm`` is "gn" or "bn"; ``tdp_nn``: the
    package's ``nn`` (native modules) or None for plain torch.nn."""
    m = tdp_nn if tdp_nn is not None else nn
    n = m.GroupNorm(4, 8) if norm == "gn" else m.BatchNorm2d(8)
    return nn.Sequential(m.Conv2d(3, 8, 3, padding=1), n, m.ReLU(), m.AdaptiveAvgPool2d((1, 1)),
                         nn.Flatten(), m.Linear(8, 4))
