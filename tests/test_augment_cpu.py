"""tdp.data.reference_augment and TrivialAugment's draws, pinned by facts that need no second
implementation (identities, shifts, rot90, a hand-computed Equalize table)."""
import numpy as np
import pytest
import torch

from tutorial_torch_distributed_data_parallel_amd.data import (AugmentedTransform,
                                                               TrivialAugment, affine_params,
                                                               augment_batch)
from tutorial_torch_distributed_data_parallel_amd.data import augment as A

fb = A.float_bits


def _img(H=12, W=12, C=3, seed=0):
    return torch.randint(0, 256, (1, H, W, C), dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(seed))


def _run(x, *row):
    return augment_batch(x, A.make_params([list(row)] * x.shape[0]))


@pytest.mark.parametrize("row", [
    (A.IDENTITY,), (A.AFFINE, 65536, 0, 0, 0, 65536, 0), (A.POSTERIZE, 8),
    (A.SOLARIZE, fb(255.5)), (A.BRIGHTNESS, fb(1.0)), (A.COLOR, fb(1.0)),
    (A.CONTRAST, fb(1.0)), (A.SHARPNESS, fb(1.0))])
@pytest.mark.parametrize("C", [1, 3])
def test_identities(row, C):
    x = _img(C=C)
    assert torch.equal(_run(x, *row), x)


def test_translate_and_rot90():
    x = _img(9, 12)
    out = _run(x, A.AFFINE, *affine_params("translate_x", 3))
    assert torch.equal(out[:, :, 3:], x[:, :, :-3]) and not out[:, :, :3].any()
    out = _run(x, A.AFFINE, *affine_params("translate_y", -2))
    assert torch.equal(out[:, :-2], x[:, 2:]) and not out[:, -2:].any()
    sq = _img(11, 11)
    assert affine_params("rotate", 90) == [0, -65536, 0, 65536, 0, 0]
    assert torch.equal(_run(sq, A.AFFINE, *affine_params("rotate", 90)),
                       torch.rot90(sq, 1, (1, 2)))


def test_autocontrast_and_equalize():
    span = _img(16, 16)
    span[0, 0, 0], span[0, 0, 1] = 0, 255
    const = torch.full((1, 8, 8, 3), 77, dtype=torch.uint8)
    for x in (span, const):
        assert torch.equal(_run(x, A.AUTOCONTRAST), x)
    assert torch.equal(_run(const, A.EQUALIZE), const)
    flat = torch.arange(256, dtype=torch.uint8).repeat(4).view(1, 32, 32, 1)  # each value 4 times
    assert torch.equal(_run(flat, A.EQUALIZE), flat)
    # two values, 512 pixels each: step = (1024 - 512) // 255 = 2, lut[10] = (0 + 1) // 2 = 0,
    # lut[200] = min(255, (512 + 1) // 2) = 255
    two = torch.tensor([10, 200], dtype=torch.uint8).repeat(512).view(1, 32, 32, 1)
    assert torch.equal(_run(two, A.EQUALIZE), torch.where(two == 10, 0, 255).to(torch.uint8))


def test_sharpness_border_and_blur():
    x = _img(7, 9)
    out = _run(x, A.SHARPNESS, fb(0.0))  # f = 0: the blurred image itself
    edge = torch.ones(7, 9, dtype=torch.bool)
    edge[1:-1, 1:-1] = False
    assert torch.equal(out[0][edge], x[0][edge])
    t = int(x[0, 2:5, 3:6, 1].long().sum() + 4 * int(x[0, 3, 4, 1]))
    assert int(out[0, 3, 4, 1]) == round(t / 13)
    assert torch.equal(_run(_img(2, 5), A.SHARPNESS, fb(1.99)), _img(2, 5))


def test_trivial_augment_draws():
    ta, tb = TrivialAugment(), TrivialAugment()
    ta.start_epoch(5), tb.start_epoch(5)
    p = ta.draw(2000, 64, 64)
    assert torch.equal(p, tb.draw(2000, 64, 64)) and not torch.equal(p, ta.draw(2000, 64, 64))
    assert p.dtype == torch.int32 and tuple(p.shape) == (2000, 8) and not p[:, 7].any()
    A._check_host_params(p)
    op, a0 = p[:, 0], p[:, 1]
    f = a0.contiguous().view(torch.float32)
    assert set(op.tolist()) == set(range(10))
    blend = torch.isin(op, torch.tensor(A._BLEND_OPS, dtype=torch.int32))
    assert 0.01 - 1e-6 <= float(f[blend].min()) and float(f[blend].max()) <= 1.99 + 1e-6
    bits = a0[op == A.POSTERIZE]
    assert 2 <= int(bits.min()) and int(bits.max()) <= 8
    thr = f[op == A.SOLARIZE]
    assert 0.0 <= float(thr.min()) and float(thr.max()) <= 255.0
    # with the nine ops above, the five affine kinds make the 14: each affine row differs from
    # the identity matrix in its own kind's entries alone (bin 0 of any kind is the identity)
    m = p[op == A.AFFINE, 1:7].double() / 65536
    off = m - torch.tensor([1.0, 0, 0, 0, 1, 0], dtype=torch.float64)
    rot = off[:, 0] != 0
    single = {"ShearX": (1, 0.99 + 1e-4), "ShearY": (3, 0.99 + 1e-4),
              "TranslateX": (2, 64.0), "TranslateY": (5, 64.0)}  # m2, m5 = -2 t, |t| <= 32
    claimed = rot.clone()
    for name, (k, top) in single.items():
        others = [c for c in range(6) if c != k]
        rows = (off[:, k] != 0) & (off[:, others] == 0).all(1)
        v = off[rows, k]
        assert len(v) and float(v.min()) < 0 < float(v.max()), name
        assert float(v.abs().max()) <= top, name
        claimed |= rows
    assert bool((claimed | (off == 0).all(1)).all())
    r = m[rot]
    assert len(r) and float(r[:, 3].min()) < 0 < float(r[:, 3].max())
    assert torch.equal(r[:, 0], r[:, 4]) and torch.equal(r[:, 1], -r[:, 3])
    assert not r[:, [2, 5]].any()
    assert float((r[:, 0] ** 2 + r[:, 3] ** 2 - 1).abs().max()) < 1e-3
    assert float(r[:, 0].min()) >= np.cos(np.radians(135)) - 1e-4
    assert len(TrivialAugment.op_names) == 14


def test_augmented_transform_forwards():
    class Inner:
        flip_p, seed = 0.25, None

        def start_epoch(self, s):
            self.seed = s

        def __call__(self, x, flip):
            return x, flip

    inner, aug = Inner(), TrivialAugment()
    t = AugmentedTransform(aug, inner)
    t.start_epoch(9)
    assert t.flip_p == 0.25 and inner.seed == 9
    x = _img(8, 8).repeat(4, 1, 1, 1)
    y, flip = t(x, "flip")
    aug.start_epoch(9)
    assert flip == "flip" and torch.equal(y, aug(x))


def test_errors():
    x, p = _img(), A.make_params([[0]])
    with pytest.raises(TypeError):
        augment_batch(x.float(), p)
    for bad_x in (x[0], _img(C=2), x.permute(0, 3, 1, 2)):
        with pytest.raises(ValueError):
            augment_batch(bad_x, p)
    for bad_p in (p[:, :7], A.make_params([[0], [0]]), A.make_params([[10]]),
                  A.make_params([[A.POSTERIZE, 9]]), A.make_params([[A.COLOR, fb(float("nan"))]])):
        with pytest.raises(ValueError):
            augment_batch(x, bad_p)
    with pytest.raises(ValueError):
        augment_batch(torch.zeros(65536, 1, 1, 1, dtype=torch.uint8), torch.zeros(65536, 8,
                                                                                 dtype=torch.int32))
    with pytest.raises(ValueError):
        affine_params("zoom", 1.0)
