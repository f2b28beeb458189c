"""tdp.data.erase_boxes (torchvision's RandomErasing rule) and CropTransform(erase=) on the CPU
path."""
import pytest
import torch

from tutorial_torch_distributed_data_parallel_amd.data import (CropTransform, RandomErasing,
                                                               crop_resize, erase_boxes)

H, W = 40, 56
SCALE, RATIO = (0.02, 0.33), (0.3, 3.3)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_erase_boxes_p0_p1_and_seed():
    assert not erase_boxes(64, H, W, p=0.0, generator=_gen(1)).any()
    b = erase_boxes(512, H, W, p=1.0, scale=SCALE, ratio=RATIO, generator=_gen(1))
    assert b.dtype == torch.int32 and b.shape == (512, 4)
    t, l, h, w = b.double().unbind(1)
    assert (h > 0).all()  # ten tries at these bounds always fit a 40 x 56 image
    assert (t >= 0).all() and (l >= 0).all() and (t + h <= H).all() and (l + w <= W).all()
    assert (h < H).all() and (w < W).all()
    # h, w are rounded: each is within 1/2 of its real value, so area and ratio keep their
    # bounds up to that half pixel per side
    assert ((h + 0.5) * (w + 0.5) >= SCALE[0] * H * W).all()
    assert ((h - 0.5) * (w - 0.5) <= SCALE[1] * H * W).all()
    assert ((h + 0.5) / (w - 0.5) >= RATIO[0]).all() and ((h - 0.5) / (w + 0.5) <= RATIO[1]).all()
    assert torch.equal(b, erase_boxes(512, H, W, p=1.0, generator=_gen(1)))
    assert not torch.equal(b, erase_boxes(512, H, W, p=1.0, generator=_gen(2)))
    half = erase_boxes(4096, H, W, p=0.5, generator=_gen(3))
    assert 0.45 < (half[:, 2] > 0).double().mean() < 0.55


def _batch():
    x = torch.randint(0, 256, (6, H, W, 3), dtype=torch.uint8, generator=_gen(7))
    flip = torch.tensor([1, 0, 1, 0, 0, 1], dtype=torch.uint8)
    return x, flip


def test_crop_transform_without_augment_is_todays_path():
    x, flip = _batch()
    tf = CropTransform(size=24, augment=None, erase=None)
    tf.start_epoch(3)
    ref = CropTransform(size=24)  # its generator, seeded alike, draws the same boxes
    ref.start_epoch(3)
    want = crop_resize(x, ref.boxes(6, H, W), flip, ref.size, ref.mean, ref.std)
    assert torch.equal(tf(x, flip), want)


@pytest.mark.parametrize("value", [0.0, (0.25, -1.5, 2.0)])
def test_crop_transform_erase_fills_the_box_only(value):
    x, flip = _batch()
    outs = []
    for p in (0.0, 1.0):
        er = RandomErasing(p=p, value=value)
        tf = CropTransform(size=24, erase=er, channels_last=False)
        tf.start_epoch(11)
        outs.append(tf(x, flip))
    er = RandomErasing(p=1.0)
    er.start_epoch(11 + 2)  # CropTransform.start_epoch's offset for the erase generator
    boxes, _ = er.draw(6, 24, 24)
    inside = torch.zeros(6, 1, 24, 24, dtype=torch.bool)
    for n, (t, l, h, w) in enumerate(boxes.tolist()):
        inside[n, :, t:t + h, l:l + w] = True
    assert inside.flatten(1).any(1).all()
    plain, erased = outs
    want = torch.tensor(value if isinstance(value, tuple) else (value,) * 3).view(1, 3, 1, 1)
    assert torch.equal(erased, torch.where(inside, want, plain))
    # the uint8 route normalises with the kernel's rule: within rounding of the one-launch path
    one = CropTransform(size=24, channels_last=False)
    one.start_epoch(11)
    assert torch.allclose(plain, one(x, flip), rtol=0, atol=1e-5)


def test_bad_arguments_raise():
    x, flip = _batch()
    b = torch.tensor([[0, 0, 8, 8]] * 6, dtype=torch.int32)
    with pytest.raises(ValueError):
        crop_resize(x, b, flip, 8, [0.0] * 3, [1.0] * 3, round_u8=False, out_dtype=torch.uint8)
    with pytest.raises(ValueError):
        CropTransform(size=8, round_u8=False, erase=RandomErasing())
