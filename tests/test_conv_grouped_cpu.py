"""Grouped convolution above the kernels: nn.Conv2d(groups=), Bottleneck(groups=, base_width=),
ResNeXt-50 32x4d, the model registry and the settings YAML -- on the CPU."""
import pytest
import torch
import yaml

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model, input_shape
from tutorial_torch_distributed_data_parallel_amd.models.resnet import Bottleneck, resnext50_32x4d
from tutorial_torch_distributed_data_parallel_amd.ops.conv import grouped_family

nn = torch.nn


def test_conv2d_groups_matches_torch_and_exchanges_state():
    torch.manual_seed(0)
    a = tdp.nn.Conv2d(8, 16, 3, groups=2)
    b = nn.Conv2d(8, 16, 3, groups=2)
    assert tuple(a.weight.shape) == (16, 4, 3, 3)
    assert a.weight.is_contiguous(memory_format=torch.channels_last)  # Cg % 4 == 0
    assert "groups=2" in repr(a)
    b.load_state_dict(a.state_dict())          # ours -> torch
    xa = torch.randn(2, 8, 9, 9, requires_grad=True)
    xb = xa.detach().clone().requires_grad_()
    ya, yb = a(xa), b(xb)
    torch.testing.assert_close(ya, yb)
    dy = torch.randn_like(ya)
    ya.backward(dy)
    yb.backward(dy)
    torch.testing.assert_close(xa.grad, xb.grad)
    torch.testing.assert_close(a.weight.grad, b.weight.grad)
    torch.testing.assert_close(a.bias.grad, b.bias.grad)
    with torch.no_grad():
        for p in b.parameters():
            p.add_(1.0)
    a.load_state_dict(b.state_dict())          # and back
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
    assert list(a.state_dict()) == list(b.state_dict()) == ["weight", "bias"]


def test_conv2d_fused_relu_and_depthwise_on_cpu():
    torch.manual_seed(1)
    a = tdp.nn.Conv2d(8, 16, 3, padding=1, groups=8, relu=True)
    x = torch.randn(2, 8, 6, 6)
    want = torch.relu(nn.functional.conv2d(x, a.weight, a.bias, 1, 1, 1, 8))
    torch.testing.assert_close(a(x), want)


def test_supported_set_is_stated():
    assert grouped_family(128, 128, 32) == "grouped"
    assert grouped_family(96, 256, 2) == "grouped"
    assert grouped_family(32, 32, 32) == "depthwise"
    assert grouped_family(8, 16, 8) == "depthwise"
    for cin, cout, groups in [(4, 4, 2), (6, 6, 6), (8, 12, 4), (64, 64, 32)]:
        with pytest.raises(NotImplementedError, match="multiples of 4"):
            grouped_family(cin, cout, groups)
    with pytest.raises(NotImplementedError, match="dilation"):
        tdp.nn.Conv2d(8, 8, 3, groups=2, dilation=2)
    assert tdp.nn.Conv2d(8, 8, 3, groups=2, dilation=[1, 1]).dilation == (1, 1)
    # a CPU module runs any combination through torch; only a GPU module refuses when built
    assert tdp.nn.Conv2d(4, 4, 3, groups=2)(torch.randn(1, 4, 5, 5)).shape == (1, 4, 3, 3)
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        tdp.nn.Conv2d(4, 4, 3, groups=2, device="cuda")
    with pytest.raises(NotImplementedError, match="dilation"):
        tdp.ops.conv2d(torch.randn(1, 8, 7, 7), torch.randn(8, 4, 3, 3), groups=2, dilation=2)


def test_default_bottleneck_is_the_dense_block():
    """Default arguments: the keys and shapes of the block as it was before ``groups`` /
    ``base_width`` existed (positional signature inplanes, planes, stride, downsample)."""
    ds = nn.Sequential(tdp.nn.Conv2d(64, 128, 1, stride=2, bias=False), tdp.nn.BatchNorm2d(128))
    blk = Bottleneck(64, 32, 2, ds)
    want = {"conv1.weight": (32, 64, 1, 1), "conv2.weight": (32, 32, 3, 3),
            "conv3.weight": (128, 32, 1, 1), "downsample.0.weight": (128, 64, 1, 1)}
    for bn, c in (("bn1", 32), ("bn2", 32), ("bn3", 128), ("downsample.1", 128)):
        want.update({f"{bn}.weight": (c,), f"{bn}.bias": (c,), f"{bn}.running_mean": (c,),
                     f"{bn}.running_var": (c,), f"{bn}.num_batches_tracked": ()})
    got = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
    assert got == want
    assert blk.conv2.groups == 1
    wide = Bottleneck(64, 64, groups=32, base_width=4)
    assert tuple(wide.conv2.weight.shape) == (128, 4, 3, 3) and wide.conv2.groups == 32
    assert tuple(wide.conv3.weight.shape) == (256, 128, 1, 1)


class _TwinBlock(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        width = int(planes * 4 / 64) * 32
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=32, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample


def _twin_resnext50(num_classes):
    """plain torch.nn ResNeXt-50 32x4d, for its parameter count and key set"""
    m = nn.Module()
    m.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    m.bn1 = nn.BatchNorm2d(64)
    inplanes = 64
    for i, (planes, blocks, stride) in enumerate([(64, 3, 1), (128, 4, 2), (256, 6, 2),
                                                  (512, 3, 2)], 1):
        ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False),
                           nn.BatchNorm2d(planes * 4))
        layer = [_TwinBlock(inplanes, planes, stride, ds)]
        inplanes = planes * 4
        layer += [_TwinBlock(inplanes, planes, 1, None) for _ in range(1, blocks)]
        setattr(m, f"layer{i}", nn.Sequential(*layer))
    m.fc = nn.Linear(2048, num_classes)
    return m


def test_resnext50_parameter_count_and_keys():
    model = resnext50_32x4d(num_classes=10)
    twin = _twin_resnext50(10)
    count = sum(p.numel() for p in model.parameters())
    assert count == sum(p.numel() for p in twin.parameters())
    # torchvision's 25,028,904 with the 1000-way head (2,049,000) replaced by a 10-way one
    assert count == 23_000_394
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == {k: tuple(v.shape) for k, v in twin.state_dict().items()}


def test_resnet50_parameter_count_did_not_move():
    from tutorial_torch_distributed_data_parallel_amd.models.resnet import resnet50

    # torchvision's 25,557,032 with the 1000-way head replaced by a 10-way one
    assert sum(p.numel() for p in resnet50(num_classes=10).parameters()) == 23_528_522


def test_build_model_resnext50_forward():
    torch.manual_seed(0)
    model = build_model("resnext50_32x4d").eval()
    with torch.no_grad():
        y = model(torch.randn(2, 3, 64, 64))
    assert y.shape == (2, 10) and bool(torch.isfinite(y).all())


def test_settings_yaml_accepts_the_name(tmp_path):
    from tutorial_torch_distributed_data_parallel_amd import cli
    from tutorial_torch_distributed_data_parallel_amd.utils.config import load_settings

    p = tmp_path / "local_settings.yaml"
    p.write_text(yaml.safe_dump({"out_dir": str(tmp_path / "out"),
                                 "train": {"model": "resnext50_32x4d", "image_size": 32,
                                           "n_train": 4, "n_test": 2}}))
    t = load_settings(str(p))["train"]
    assert input_shape(t["model"], t["image_size"]) == (3, 32, 32)
    train, test = cli._datasets(t, torch.device("cpu"))
    assert len(train) == 4 and len(test) == 2
    model = build_model(t["model"])
    assert model.layer1[0].conv2.groups == 32
