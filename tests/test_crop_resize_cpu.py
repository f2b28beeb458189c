"""Crop-box samplers and crop_resize's CPU path (float64 oracle as in test_crop_resize_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

from tutorial_torch_distributed_data_parallel_amd.data import (center_crop_boxes, crop_resize,
                                                               pad_crop_boxes, resized_crop_boxes)


def gen(seed=0):
    return torch.Generator().manual_seed(seed)


def test_resized_crop_boxes_inside_and_within_bounds():
    H, W, scale, ratio = 48, 64, (0.08, 1.0), (3 / 4, 4 / 3)
    t, l, h, w = resized_crop_boxes(4000, H, W, scale, ratio, gen()).double().unbind(1)
    assert resized_crop_boxes(7, H, W).dtype == torch.int32
    assert (t >= 0).all() and (l >= 0).all() and (t + h <= H).all() and (l + w <= W).all()
    assert (h >= 1).all() and (w >= 1).all()
    # w, h are rounded: each is within half a pixel of sqrt(area * r), sqrt(area / r)
    lo, hi = (w - 0.5).clamp(min=0) * (h - 0.5).clamp(min=0), (w + 0.5) * (h + 0.5)
    assert (hi >= scale[0] * H * W).all() and (lo <= scale[1] * H * W).all()
    assert ((w + 0.5) / (h - 0.5) >= ratio[0]).all() and ((w - 0.5) / (h + 0.5) <= ratio[1]).all()
    assert t.unique().numel() > 10 and w.unique().numel() > 10


def test_resized_crop_boxes_fallback():
    # 1024 * 3 of area cannot fit: central crop at the nearest allowed ratio, w = 32, h = 32 / 3
    b = resized_crop_boxes(5, 32, 32, scale=(1.0, 1.0), ratio=(3.0, 3.0), generator=gen())
    assert b.tolist() == [[10, 0, 11, 32]] * 5
    b = resized_crop_boxes(5, 32, 48, scale=(4.0, 4.0), generator=gen())  # ratio 1.5 > 4/3
    assert b.tolist() == [[0, 2, 32, 43]] * 5


def test_pad_and_center_crop_boxes():
    b = pad_crop_boxes(2000, 32, 32, 32, 4, gen())
    assert b.dtype == torch.int32 and (b[:, 2:] == 32).all()
    for k in (0, 1):  # [-p, H + p - size] = [-4, 4], both ends reached
        assert b[:, k].min() == -4 and b[:, k].max() == 4
    assert center_crop_boxes(3, 256, 256).tolist() == [[16, 16, 224, 224]] * 3


def test_same_seed_same_boxes():
    assert torch.equal(resized_crop_boxes(50, 40, 40, generator=gen(3)),
                       resized_crop_boxes(50, 40, 40, generator=gen(3)))
    assert torch.equal(pad_crop_boxes(50, 32, 32, 32, 4, gen(3)),
                       pad_crop_boxes(50, 32, 32, 32, 4, gen(3)))


@pytest.mark.parametrize("Hs,Ws,boxes,size,fill", [
    (40, 32, [(1, 2, 37, 29), (0, 0, 40, 32)], (8, 8), 0.0),
    (16, 16, [(-3, -2, 12, 12), (9, 9, 10, 5)], (19, 21), 128.0),
])
def test_crop_resize_cpu_matches_float64(Hs, Ws, boxes, size, fill):
    x = torch.randint(0, 256, (2, Hs, Ws, 3), generator=gen(), dtype=torch.uint8)
    boxes, flip = torch.tensor(boxes, dtype=torch.int32), torch.tensor([0, 1], dtype=torch.uint8)
    out = crop_resize(x, boxes, flip, size, [0.0] * 3, [1 / 255] * 3, round_u8=False, fill=fill)
    assert out.is_contiguous(memory_format=torch.channels_last)
    xp = F.pad(x.permute(0, 3, 1, 2).double(), (16, 16, 16, 16), value=fill)
    ref = torch.cat([F.interpolate(xp[b:b + 1, :, t + 16:t + 16 + h, l + 16:l + 16 + w], size=size,
                                   mode="bilinear", antialias=True, align_corners=False)
                     for b, (t, l, h, w) in enumerate(boxes.tolist())])
    ref[1] = ref[1].flip(-1)
    # fp32 filtering of values <= 255 with at most ceil(2 * 37 / 8) + 1 = 11 taps per axis
    assert (out.double() - ref).abs().max() <= 255 * (11 + 11 + 8) * 2.0 ** -24
    with pytest.raises(ValueError):
        crop_resize(x, torch.tensor([[0, 0, 0, 4], [0, 0, 4, 4]], dtype=torch.int32), None, size,
                    [0.0] * 3, [1.0] * 3)
