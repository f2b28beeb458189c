"""GroupNorm on the CPU: ``ops.group_norm`` against ``F.group_norm`` under autograd, the
``tdp.nn.GroupNorm`` module, ``resnet50_gn`` against its hand-written torch.nn twin, the
``norm_layer`` refactor of ResNet (``resnet50()`` unchanged), the registry, and the property the
op exists for: a data-parallel step does not depend on how the batch is split over the ranks."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops
from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model, input_shape
from tutorial_torch_distributed_data_parallel_amd.models.resnet import (ResNet, resnet50,
                                                                         resnet50_gn)
from tutorial_torch_distributed_data_parallel_amd.parallel.launcher import spawn

import groupnorm_workers as W  # noqa: E402  (tests/ is on sys.path via conftest)
from groupnorm_twin import TwinResNetGN


def _inputs(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    return (torch.randn(shape, generator=g), torch.empty(C).uniform_(0.5, 2, generator=g),
            torch.empty(C).uniform_(-1, 1, generator=g), torch.randn(shape, generator=g),
            torch.randn(shape, generator=g))


@pytest.mark.parametrize("shape, G", [((2, 8, 3, 3), 2), ((3, 6, 5), 3), ((4, 12), 3),
                                      ((2, 6, 5, 5), 6)])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("residual", [False, True])
def test_op_matches_torch_under_autograd(shape, G, affine, relu, residual):
    x, w, b, res, dy = _inputs(shape)
    mine = [t.clone().requires_grad_() for t in (x, w, b, res)]
    refs = [t.clone().requires_grad_() for t in (x, w, b, res)]
    y = ops.group_norm(mine[0], G, mine[1] if affine else None, mine[2] if affine else None,
                       relu=relu, residual=mine[3] if residual else None)
    z = F.group_norm(refs[0], G, refs[1] if affine else None, refs[2] if affine else None)
    z = z + refs[3] if residual else z
    z = F.relu(z) if relu else z
    if not relu and not residual:
        assert torch.equal(y, z)  # the plain case is F.group_norm itself
    torch.testing.assert_close(y, z)
    y.backward(dy)
    z.backward(dy)
    used = [0] + ([1, 2] if affine else []) + ([3] if residual else [])
    for i in used:
        torch.testing.assert_close(mine[i].grad, refs[i].grad)
    for i in set(range(4)) - set(used):
        assert mine[i].grad is None


def test_shape_and_flag_errors():
    with pytest.raises(ValueError, match="not divisible"):
        ops.group_norm(torch.randn(2, 6, 3, 3), 4)
    with pytest.raises(ValueError, match="at least 2D"):
        ops.group_norm(torch.randn(8), 2)
    with pytest.raises(ValueError, match="residual"):
        ops.group_norm(torch.randn(2, 4, 3), 2, residual=torch.randn(2, 4, 2))
    assert "group_norm" in ops.__all__ and "GroupNorm" in tdp.nn.__all__


def test_module_is_torchs_with_a_fused_relu_and_join():
    torch.manual_seed(0)
    m, t = tdp.nn.GroupNorm(4, 8), nn.GroupNorm(4, 8)
    assert isinstance(m, nn.GroupNorm)
    assert {k: v.shape for k, v in m.state_dict().items()} == \
        {k: v.shape for k, v in t.state_dict().items()}
    assert list(m.state_dict()) == ["weight", "bias"] and not list(m.buffers())
    assert bool((m.weight == 1).all()) and not m.bias.any()
    assert repr(m) == repr(t)
    assert "relu=True" in repr(tdp.nn.GroupNorm(4, 8, relu=True))
    nn.init.uniform_(m.weight, 0.5, 2)
    nn.init.uniform_(m.bias, -1, 1)
    t.load_state_dict(m.state_dict())
    x, r = torch.randn(3, 8, 5, 5), torch.randn(3, 8, 5, 5)
    assert torch.equal(m(x), t(x))
    assert torch.equal(m.eval()(x), t(x))  # no running statistics: eval is the same computation
    m.train()
    torch.testing.assert_close(m.relu_join(x, r), F.relu(t(x) + r))
    torch.testing.assert_close(m(x, relu=True), F.relu(t(x)))
    mr = tdp.nn.GroupNorm(4, 8, relu=True)
    mr.load_state_dict(m.state_dict())
    torch.testing.assert_close(mr(x), F.relu(t(x)))
    assert torch.equal(mr(x, relu=False), t(x))
    na = tdp.nn.GroupNorm(2, 8, affine=False, eps=1e-3)
    assert na.weight is None and na.bias is None and not na.state_dict()
    assert torch.equal(na(x), F.group_norm(x, 2, None, None, 1e-3))


def test_convert_sync_batchnorm_leaves_group_norm_alone():
    seq = nn.Sequential(tdp.nn.Conv2d(3, 8, 1), tdp.nn.BatchNorm2d(8, relu=True),
                        tdp.nn.GroupNorm(4, 8, relu=True), nn.GroupNorm(2, 8), nn.BatchNorm2d(8))
    gn_native, gn_torch = seq[2], seq[3]
    conv = tdp.nn.convert_sync_batchnorm(seq)
    assert isinstance(conv[1], tdp.nn.SyncBatchNorm) and isinstance(conv[4], tdp.nn.SyncBatchNorm)
    assert conv[2] is gn_native and conv[3] is gn_torch
    assert type(conv[2]) is tdp.nn.GroupNorm and conv[2].relu


def _count(m):
    return sum(p.numel() for p in m.parameters())


def test_resnet50_gn_is_torchvisions_network():
    m, t = resnet50_gn(num_classes=1000), TwinResNetGN(num_classes=1000)
    sd, td = m.state_dict(), t.state_dict()
    assert list(sd) == list(td)
    assert all(sd[k].shape == td[k].shape for k in sd)
    assert len(sd) == 161 == len(list(m.parameters()))
    assert _count(m) == 25_557_032 == _count(t)
    assert not list(m.buffers())
    for k in ("bn1.weight", "layer1.0.bn3.bias", "layer1.0.downsample.1.weight",
              "layer4.2.bn2.weight", "fc.bias"):
        assert k in sd, k
    norms = [g for g in m.modules() if isinstance(g, nn.GroupNorm)]
    assert len(norms) == 53 and all(type(g) is tdp.nn.GroupNorm and g.num_groups == 32
                                    for g in norms)
    assert all(bool((g.weight == 1).all()) and not g.bias.any() for g in norms)
    assert not any(isinstance(b, nn.modules.batchnorm._BatchNorm) for b in m.modules())
    convs = [c for c in m.modules() if isinstance(c, nn.Conv2d)]
    assert len(convs) == 53 and not any(c.bn_stats for c in convs)
    # the fused ReLUs sit where the BatchNorm network has them
    assert m.bn1.relu and m.layer1[0].bn1.relu and m.layer1[0].bn2.relu
    assert not m.layer1[0].bn3.relu and not m.layer1[0].downsample[1].relu
    assert hasattr(m.layer1[0].bn3, "relu_join")
    assert resnet50_gn(groups=16).layer2[1].bn2.num_groups == 16


def test_registry_and_settings(tmp_path):
    from tutorial_torch_distributed_data_parallel_amd.utils import config

    m = build_model("resnet50_gn")
    assert isinstance(m, ResNet) and m.fc.out_features == 10
    assert isinstance(m.bn1, tdp.nn.GroupNorm)
    assert input_shape("resnet50_gn") == (3, 224, 224)
    path = tmp_path / "settings.yaml"
    path.write_text("train:\n  model: resnet50_gn\n")
    cfg = config.load_settings(str(path))
    assert cfg["train"]["model"] == "resnet50_gn"
    m = build_model(cfg["train"]["model"], num_classes=7).eval()
    with torch.no_grad():
        y = m(torch.randn(2, 3, 32, 32))
    assert y.shape == (2, 7) and bool(torch.isfinite(y).all())


def cut_down_pair(dtype=torch.float32, device="cpu"):
    """``resnet50_gn`` at one block per stage and its twin with the same weights (affine pairs
    moved off 1 / 0 so that their gradients' formulas are exercised)."""
    torch.manual_seed(0)

    def norm(c, relu=False, device=None):
        return tdp.nn.GroupNorm(32, c, relu=relu, device=device)

    m = ResNet((1, 1, 1, 1), num_classes=10, norm_layer=norm)
    for g in m.modules():
        if isinstance(g, nn.GroupNorm):
            nn.init.uniform_(g.weight, 0.5, 1.5)
            nn.init.uniform_(g.bias, -0.5, 0.5)
    t = TwinResNetGN((1, 1, 1, 1), num_classes=10)
    assert list(m.state_dict()) == list(t.state_dict())
    t.load_state_dict(m.state_dict())
    return m.to(device=device, dtype=dtype), t.to(device=device, dtype=dtype)


@pytest.mark.parametrize("fused", [True, False])
def test_cut_down_model_matches_its_twin(fused):
    m, t = cut_down_pair()
    for b in m.modules():
        if hasattr(b, "_fused_join"):
            b._fused_join = fused
    x = torch.randn(2, 3, 32, 32)
    xm, xt = x.clone().requires_grad_(), x.clone().requires_grad_()
    y, yt = m(xm), t(xt)
    torch.testing.assert_close(y, yt, rtol=1e-4, atol=1e-5)
    y.square().sum().backward()
    yt.square().sum().backward()
    torch.testing.assert_close(xm.grad, xt.grad, rtol=1e-3, atol=1e-4)
    for (n, p), q in zip(m.named_parameters(), t.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-3, atol=1e-4,
                                   msg=lambda s: f"{n}: {s}")


def test_resnet50_is_unchanged_by_the_norm_layer_argument():
    """Same module types, keys and initial values as the construction the argument replaced:
    BatchNorm2d everywhere (fused ReLU on bn1 / bn2), every convolution asked for its batch
    statistics, and the seed-0 weights of a direct torch construction in the same order."""
    torch.manual_seed(0)
    m = resnet50()
    kinds = [type(x).__name__ for x in m.modules()]
    assert kinds.count("BatchNorm2d") == 53 and kinds.count("Conv2d") == 53
    assert kinds.count("GroupNorm") == 0 and kinds.count("Bottleneck") == 16
    assert all(type(b) is tdp.nn.BatchNorm2d for b in m.modules()
               if isinstance(b, nn.modules.batchnorm._BatchNorm))
    assert all(c.bn_stats for c in m.modules() if isinstance(c, nn.Conv2d))
    assert m.bn1.relu and m.layer3[2].bn2.relu and not m.layer3[2].bn3.relu
    assert not hasattr(m, "_norm_layer")
    sd = m.state_dict()
    assert len(sd) == 161 + 53 * 3 and len(list(m.parameters())) == 161
    assert _count(m) == 23_528_522
    assert "layer4.2.bn3.running_var" in sd and "layer1.0.downsample.1.num_batches_tracked" in sd
    # initial values: the torch.nn twin built under the same seed and initialised by torchvision's
    # loop consumes the generator identically (normalisation layers draw nothing)
    torch.manual_seed(0)
    t = TwinResNetGN()
    for c in t.modules():
        if isinstance(c, nn.Conv2d):
            if c.in_channels % 4 == 0:  # the native Conv2d keeps its weight channels_last
                c.weight.data = c.weight.data.contiguous(memory_format=torch.channels_last)
            nn.init.kaiming_normal_(c.weight, mode="fan_out", nonlinearity="relu")
    td = t.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean") or k.endswith("num_batches_tracked"):
            assert not v.any(), k
        elif k.endswith("running_var"):
            assert bool((v == 1).all()), k
        else:
            assert torch.equal(v, td[k]), k  # convs and fc drawn alike; gamma 1, beta 0
    w = sd["layer2.0.conv2.weight"]  # Kaiming-normal fan_out: std = sqrt(2 / (128 * 9))
    assert abs(w.std().item() / (2.0 / (128 * 9)) ** 0.5 - 1) < 0.02
    assert bool((sd["layer2.0.bn3.weight"] == 1).all()) and not sd["layer2.0.bn3.bias"].any()
    assert isinstance(build_model("resnext50_32x4d").layer1[0].bn2, tdp.nn.BatchNorm2d)


def test_group_norm_ddp_step_does_not_depend_on_the_split():
    spawn(W.split_batch_step, 2, args=("gn", True), grace=5.0)


def test_batch_norm_ddp_step_without_syncbn_does_depend_on_it():
    spawn(W.split_batch_step, 2, args=("bn", False), grace=5.0)
