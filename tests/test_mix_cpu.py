"""BatchMix's draws and the CPU paths of mix_batch / cross_entropy_pair / probability targets."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.ops.loss import pair_target


def _draws(mix, seed, k=6):
    mix.start_epoch(seed)
    return [mix.draw(8, 32, 24) for _ in range(k)]


def test_batchmix_is_deterministic_per_seed():
    mix = tdp.data.BatchMix()
    a, b, c = _draws(mix, 11), _draws(mix, 11), _draws(mix, 12)
    assert all(torch.equal(u, v) for da, db in zip(a, b) for u, v in zip(da, db))
    assert any(not torch.equal(u, v) for da, dc in zip(a, c) for u, v in zip(da, dc))


@pytest.mark.parametrize("seed", range(5))
def test_cutmix_lam_is_the_clipped_area(seed):
    mix = tdp.data.BatchMix(mixup_alpha=0.0, cutmix_alpha=1.0)
    H, W = 32, 24
    for perm, lam_x, boxes, lam_y in _draws(mix, seed):
        assert sorted(perm.tolist()) == list(range(8)) and bool((lam_x == 1).all())
        t, l, h, w = boxes[0].tolist()
        assert bool((boxes == boxes[0]).all()) and 0 <= t and t + h <= H and 0 <= l and l + w <= W
        assert bool((lam_y == float(np.float32(1.0 - h * w / (H * W)))).all())


def test_mixup_and_identity_draws():
    for perm, lam_x, boxes, lam_y in _draws(tdp.data.BatchMix(0.2, 0.0), 1):
        assert torch.equal(lam_x, lam_y) and not boxes.any() and 0 <= lam_x[0] <= 1
    for perm, lam_x, boxes, lam_y in _draws(tdp.data.BatchMix(prob=0.0), 1):
        assert bool((lam_x == 1).all()) and bool((lam_y == 1).all()) and not boxes.any()


def test_cpu_paths_equal_the_torch_composition():
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(4, 3, 6, 5, generator=gen)
    y = torch.randint(0, 7, (4,), generator=gen)
    mix = tdp.data.BatchMix(0.0, 1.0)
    mix.start_epoch(5)
    perm, lam_x, boxes, lam_y = mix.draw(4, 6, 5)
    mix.start_epoch(5)
    out, (ya, yb, lam) = mix(x, y)
    t, l, h, w = boxes[0].tolist()
    want = x.clone()
    want[:, :, t:t + h, l:l + w] = x[perm.long()][:, :, t:t + h, l:l + w]
    assert torch.equal(out, want) and torch.equal(yb, y[perm.long()]) and torch.equal(lam, lam_y)
    lam2 = torch.tensor([0.3, 1.0, 0.0, 0.6])
    got = tdp.data.mix_batch(x, perm, lam2, torch.zeros(4, 4, dtype=torch.int32))
    lv = lam2.view(4, 1, 1, 1)
    assert torch.equal(got, torch.where(lv == 1, x, lv * x + (1 - lv) * x[perm.long()]))
    z = torch.randn(4, 7, generator=gen, requires_grad=True)
    dense = pair_target(ya, yb, lam2, 7)
    acc, acc2 = torch.zeros(3), torch.zeros(3)
    loss = tdp.ops.cross_entropy_pair(z, ya, yb, lam2, label_smoothing=0.1, acc=acc)
    assert torch.equal(loss, F.cross_entropy(z, dense, label_smoothing=0.1))
    assert torch.equal(loss, tdp.ops.cross_entropy(z, dense, label_smoothing=0.1, acc=acc2))
    assert torch.equal(loss, tdp.nn.CrossEntropyLoss(label_smoothing=0.1)(z, dense))
    assert torch.equal(acc, acc2) and acc[2] == 4


def test_refusals():
    z, y = torch.randn(4, 7), torch.zeros(4, dtype=torch.int64)
    lam = torch.ones(4)
    with pytest.raises(TypeError):
        tdp.ops.cross_entropy(z, y.int())
    with pytest.raises(ValueError):
        tdp.ops.cross_entropy(z, torch.rand(4, 6))
    with pytest.raises(ValueError):
        tdp.ops.cross_entropy(z, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError):
        tdp.ops.cross_entropy_pair(z, y.int(), y, lam)
    with pytest.raises(ValueError):
        tdp.ops.cross_entropy_pair(z, y, y[:3], lam)
    x, boxes = torch.randn(4, 3, 5, 5), torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(TypeError):
        tdp.data.mix_batch(x, y, lam, boxes.long())
    with pytest.raises(ValueError):
        tdp.data.mix_batch(x, y[:3], lam, boxes)
    with pytest.raises(ValueError):
        tdp.data.mix_batch(x.requires_grad_(), y, lam, boxes)
