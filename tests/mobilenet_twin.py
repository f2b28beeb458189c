"""MobileNetV2 in plain torch.nn, module for module torchvision's ``mobilenet_v2`` (same
``state_dict`` keys: the ReLU6 of a conv-BN-ReLU6 triple sits at index 2 and has no parameters):
the twin the MobileNetV2 tests compare ``models/mobilenet.py`` against, so a ``state_dict`` of
either loads into the other."""
import torch.nn as nn


def make_divisible(v, divisor=8, min_value=None):
    if min_value is None:
        min_value = divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def conv_bn_relu6(cin, cout, kernel=3, stride=1, groups=1):
    return nn.Sequential(
        nn.Conv2d(cin, cout, kernel, stride, (kernel - 1) // 2, groups=groups, bias=False),
        nn.BatchNorm2d(cout), nn.ReLU6())


class TwinInvertedResidual(nn.Module):
    def __init__(self, inp, oup, stride, t):
        super().__init__()
        hidden = int(round(inp * t))
        self.use_res_connect = stride == 1 and inp == oup
        layers = []
        if t != 1:
            layers.append(conv_bn_relu6(inp, hidden, 1))
        layers += [conv_bn_relu6(hidden, hidden, 3, stride, groups=hidden),
                   nn.Conv2d(hidden, oup, 1, 1, 0, bias=False), nn.BatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.use_res_connect else self.conv(x)


SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1),
           (6, 160, 3, 2), (6, 320, 1, 1))


class TwinMobileNetV2(nn.Module):
    def __init__(self, num_classes=10, width_mult=1.0, dropout=0.2):
        super().__init__()
        inp = make_divisible(32 * width_mult)
        last = make_divisible(1280 * max(1.0, width_mult))
        features = [conv_bn_relu6(3, inp, 3, 2)]
        for t, c, n, s in SETTING:
            oup = make_divisible(c * width_mult)
            for i in range(n):
                features.append(TwinInvertedResidual(inp, oup, s if i == 0 else 1, t))
                inp = oup
        features.append(conv_bn_relu6(inp, last, 1))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(nn.Dropout(dropout), nn.Linear(last, num_classes))

    def forward(self, x):
        x = self.features(x)
        x = nn.functional.adaptive_avg_pool2d(x, (1, 1))
        return self.classifier(x.flatten(1))


U = 2.0 ** -24


def grad_scales(ref_model):
    """max |gradient| per parameter of the float64 twin, taken over the parameters of the same
    module: the bias of a BatchNorm that feeds a 1x1 convolution + BatchNorm has an exactly zero
    gradient (a per-channel constant is removed by the next mean subtraction), computed as a sum
    of terms of the size of its weight's -- its rounding noise scales with those, not with 0."""
    out = {}
    for mn, mod in ref_model.named_modules():
        ps = [(n, p) for n, p in mod.named_parameters(recurse=False) if p.grad is not None]
        if ps:
            sc = max(p.grad.abs().max().item() for _, p in ps)
            for n, _ in ps:
                out[f"{mn}.{n}" if mn else n] = sc
    return out


def check_rule(what, got, t32, ref, scale, c=2):
    """The project's tolerance rule (tests/test_hard_inputs_gpu.py) for one quantity against a
    float64 reference: e_k <= 4 e_t + c 2^-24 scale, e_t torch's own fp32 error."""
    e_k = (got.detach().double().cpu() - ref.detach().cpu()).abs().max().item()
    e_t = (t32.detach().double().cpu() - ref.detach().cpu()).abs().max().item()
    bound = 4 * e_t + c * U * scale
    print(f"[rule] {what}: e_k={e_k:.3e} e_t={e_t:.3e} scale={scale:.3e} bound={bound:.3e}")
    assert e_k <= bound, f"{what}: e_k {e_k:.3e} > 4 * {e_t:.3e} + {c} * 2^-24 * {scale:.3e}"
    return e_k, e_t


def check_grads_rule(tag, model, t32, t64, c=2):
    scales = grad_scales(t64)
    for (n, p), q, r in zip(model.named_parameters(), t32.parameters(), t64.parameters()):
        check_rule(f"{tag} d{n}", p.grad, q.grad, r.grad, scales[n], c)
