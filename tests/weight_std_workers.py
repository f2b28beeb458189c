"""Oracles of the weight-standardisation tests in plain ``torch.nn``: the formula, a convolution
on the composed weight, ResNet-50 GN+WS as a twin, and the worker of the two-rank gloo step
(run under parallel.launcher.spawn)."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.parallel import runtime as rt

from groupnorm_twin import TwinResNetGN


def compose(w, eps=1e-5):
    """The issue's formula in ``w``'s own dtype and memory layout."""
    mean = w.mean(dim=(1, 2, 3), keepdim=True)
    var = (w - mean).square().mean(dim=(1, 2, 3), keepdim=True)
    return (w - mean) * torch.rsqrt(var + eps)


class TwinStdConv2d(nn.Conv2d):
    def forward(self, x):
        return self._conv_forward(x, compose(self.weight), self.bias)


def twin_resnet(layers, num_classes=10):
    t = TwinResNetGN(layers, num_classes=num_classes)
    for c in t.modules():
        if type(c) is nn.Conv2d:
            c.__class__ = TwinStdConv2d
    return t


def cut_down_pair():
    """``resnet50_gn_ws`` at one block per stage and its twin with the same weights."""
    from tutorial_torch_distributed_data_parallel_amd.models.resnet import ResNet

    torch.manual_seed(0)
    m = ResNet((1, 1, 1, 1), num_classes=10, conv_layer=tdp.nn.StdConv2d,
               norm_layer=lambda c, relu=False, device=None: tdp.nn.GroupNorm(32, c, relu=relu))
    t = twin_resnet((1, 1, 1, 1))
    t.load_state_dict(m.state_dict())
    return m, t


def small_net(native: bool):
    conv = tdp.nn.StdConv2d if native else TwinStdConv2d
    m = tdp.nn if native else nn
    return nn.Sequential(conv(3, 8, 3, padding=1), m.GroupNorm(4, 8), m.ReLU(),
                         conv(8, 8, 1, bias=False), m.AdaptiveAvgPool2d((1, 1)), nn.Flatten(),
                         m.Linear(8, 4))


def split_batch_step(rank):
    """The net under 2-rank tdp.DDP, a batch of 8 split 4 + 4, one SGD step, against the
    single-process step of the torch.nn twin on the full batch."""
    torch.set_num_threads(2)
    tdp.init_process_group("gloo")
    r, ws = rt.get_rank(), rt.get_world_size()
    torch.manual_seed(0)
    model, ref = small_net(True), small_net(False)
    ref.load_state_dict(copy.deepcopy(model.state_dict()))
    g = torch.Generator().manual_seed(11)
    X, Y = torch.randn(8, 3, 6, 6, generator=g), torch.randint(0, 4, (8,), generator=g)
    lr = 0.1
    F.cross_entropy(ref(X), Y).backward()
    with torch.no_grad():
        for p in ref.parameters():
            p -= lr * p.grad
    ddp = tdp.DDP(model)
    opt = tdp.optim.SGD(model.parameters(), lr=lr)
    per = 8 // ws
    tdp.ops.cross_entropy(ddp(X[r * per:(r + 1) * per]), Y[r * per:(r + 1) * per]).backward()
    opt.step()
    for (n, p), q in zip(model.named_parameters(), ref.parameters()):
        torch.testing.assert_close(p.detach(), q.detach(), msg=lambda s: f"{n}: {s}")
    tdp.destroy_process_group()
