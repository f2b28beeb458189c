"""image_crop_resize (csrc/image_crop.hip) against a float64 CPU oracle: pad with fill, slice the
box, F.interpolate(double, antialias=True), flip. mean = 0, std = 1/255: outputs are grey levels."""
import pytest
import torch
import torch.nn.functional as F

from tutorial_torch_distributed_data_parallel_amd import _native
from tutorial_torch_distributed_data_parallel_amd.data import (CropTransform, ImageTransform,
                                                               PrefetchLoader, cifar_like_uint8,
                                                               crop_resize)

pytestmark = pytest.mark.gpu
FLIP = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)


def oracle(x, boxes, flip, size, fill=0.0, rounded=False):
    H, W = x.shape[1:3]
    p = max(0, int(-boxes[:, :2].min()), int((boxes[:, 0] + boxes[:, 2]).max()) - H,
            int((boxes[:, 1] + boxes[:, 3]).max()) - W)
    xp = F.pad(x.permute(0, 3, 1, 2).double(), (p, p, p, p), value=fill)
    y = torch.cat([F.interpolate(xp[b:b + 1, :, t + p:t + p + h, l + p:l + p + w], size=size,
                                 mode="bilinear", antialias=True, align_corners=False)
                   for b, (t, l, h, w) in enumerate(boxes.tolist())])
    y = y.round() if rounded else y
    return torch.where(flip.bool().view(-1, 1, 1, 1), y.flip(-1), y)


def max_taps(n_in, n_out):
    s = n_in / n_out
    sup = max(s, 1.0)
    return max(min(n_in, int((o + 0.5) * s + sup + 0.5)) - max(0, int((o + 0.5) * s - sup + 0.5))
               for o in range(n_out))


def tolerance(boxes, size):
    th = max(max_taps(int(h), size[0]) for h in boxes[:, 2])
    tw = max(max_taps(int(w), size[1]) for w in boxes[:, 3])
    return 255.0 * (th + tw + 8) * 2.0 ** -24


def run(x, boxes, flip, size, C, channels_last=True, round_u8=False, fill=0.0):
    out = crop_resize(x.cuda(), boxes.cuda(), None if flip is None else flip.cuda(), size,
                      [0.0] * C, [1 / 255] * C, round_u8, channels_last, fill)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    assert out.shape == (len(x), C, *size) and out.is_contiguous(memory_format=fmt)
    return out.cpu()


def same(box):
    return [box] * 5


# boxes over the corner, top, left, bottom and right edge of a 16x16 source
EDGES = [(-3, -2, 12, 12), (-3, 2, 10, 10), (2, -2, 10, 10), (9, 3, 10, 10), (3, 9, 10, 10)]
# name: (Hs, Ws, five boxes (top, left, h, w), output size, fill)
CASES = {
    "down_37x29_to_8": (40, 32, same((1, 2, 37, 29)), (8, 8), 0.0),
    "up_5x7_to_19x21": (16, 16, same((4, 3, 5, 7)), (19, 21), 0.0),  # tile tails on both axes
    "box_1x1": (9, 9, same((4, 5, 1, 1)), (6, 6), 0.0),
    "edges_fill0": (16, 16, EDGES, (9, 11), 0.0),
    "edges_fill128": (16, 16, EDGES, (9, 11), 128.0),
    # the one tile's vertical taps span all 200 box rows: several chunks of CROP_STAGE_ROWS (64)
    "chunked_200_to_7": (208, 204, same((3, 2, 200, 200)), (7, 7), 0.0),
    "mixed_boxes": (40, 40, [(0, 0, 37, 29), (3, 5, 20, 33), (-2, -3, 11, 9), (10, 10, 1, 1),
                             (0, 0, 40, 40)], (17, 18), 0.0),
    "up_32_to_224": (32, 32, same((0, 0, 32, 32)), (224, 224), 0.0),
}


def inputs(name, C):
    Hs, Ws, boxes, size, fill = CASES[name]
    g = torch.Generator().manual_seed(len(name) * 7 + C)
    x = torch.randint(0, 256, (5, Hs, Ws, C), generator=g, dtype=torch.uint8)
    return x, torch.tensor(boxes, dtype=torch.int32), size, fill


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_unrounded_matches_float64(name, C, channels_last):
    x, boxes, size, fill = inputs(name, C)
    if name.startswith("chunked"):
        assert 200 > _native.native().CROP_STAGE_ROWS and size[0] <= _native.native().CROP_TILE
    out = run(x, boxes, FLIP, size, C, channels_last, fill=fill)
    err = (out.double() - oracle(x, boxes, FLIP, size, fill)).abs().max().item()
    tol = tolerance(boxes, size)
    print(f"{name} C={C} cl={channels_last}: max err {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("C", [1, 3, 4])
def test_identity_is_bitwise_the_pixels(C):
    x, _, _, _ = inputs("up_32_to_224", C)
    boxes = torch.tensor(same((0, 0, 32, 32)), dtype=torch.int32)
    out = run(x, boxes, None, (32, 32), C)
    # the kernel's normalisation of the exact pixel value, in fp32: (v * (1/255)) * 255
    want = (x.permute(0, 3, 1, 2).float() * (torch.tensor(1.0) / 255.0)) * 255.0
    assert torch.equal(out, want) and torch.equal(out.round(), x.permute(0, 3, 1, 2).float())


def test_upscale_agrees_with_image_transform():
    """image_transform forms its sample position in fp32: (o + 0.5) * (32 / 224) - 0.5 carries up
    to half an ulp of 32 plus 223.5 times the rounding of 32/224, about 3.3e-6 pixels per axis,
    which moves its value by that times the local slope. The bound below only covers fp32
    accumulation, so this image is a ramp whose neighbouring pixels differ by at most 6 grey
    levels (position error <= 2 * 6 * 3.3e-6 = 4e-5); the noisy 32 -> 224 image is held to float64
    in test_unrounded_matches_float64."""
    i = torch.arange(32)
    x = (3 * i.view(1, 32, 1, 1) + 4 * i.view(1, 1, 32, 1) + 10 * torch.arange(3).view(1, 1, 1, 3)
         + torch.arange(5).view(5, 1, 1, 1) % 3).to(torch.uint8).contiguous()
    boxes = torch.tensor(same((0, 0, 32, 32)), dtype=torch.int32)
    out = run(x, boxes, FLIP, (224, 224), 3)
    tf = ImageTransform(size=224, mean=[0.0] * 3, std=[1 / 255] * 3, round_u8=False)
    err = (out - tf(x.cuda(), FLIP.cuda()).cpu()).abs().max().item()
    print(f"crop_resize vs image_transform: max err {err:.3e}")
    assert err <= tolerance(boxes, (224, 224))


@pytest.mark.parametrize("name", ["chunked_200_to_7", "mixed_boxes"])
def test_two_runs_bitwise_equal(name):
    x, boxes, size, _ = inputs(name, 3)
    assert torch.equal(run(x, boxes, FLIP, size, 3), run(x, boxes, FLIP, size, 3))


@pytest.mark.parametrize("name", ["down_37x29_to_8", "up_5x7_to_19x21"])
def test_rounded_within_one_grey_level(name):
    x, boxes, size, _ = inputs(name, 3)
    d = (run(x, boxes, FLIP, size, 3, round_u8=True).double()
         - oracle(x, boxes, FLIP, size, rounded=True)).abs()
    print(f"{name}: {int((d > 0.5).sum())} of {d.numel()} pixels differ")
    assert d.max() <= 1.0 + 1e-4 and (d > 0.5).double().mean() < 1e-3


def test_bad_boxes_raise():
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8).cuda()
    for bad in (torch.tensor([[0, 0, 0, 4], [0, 0, 4, 4]], dtype=torch.int32).cuda(),
                torch.tensor([[0, 0, 4, 4]], dtype=torch.int32).cuda(),
                torch.tensor([[0, 0, 4, 4], [0, 0, 4, 4]]).cuda()):
        with pytest.raises((RuntimeError, ValueError)):
            crop_resize(x, bad, None, 4, [0.0] * 3, [1.0] * 3)


def test_prefetch_loader_random_pad_crop():
    ds = cifar_like_uint8(n=256)

    def epochs(n, seed=5):  # flip_p = 0: the batches differ by their crops alone
        tf = CropTransform(size=32, crop="random_pad", padding=4, flip_p=0.0)
        loader = PrefetchLoader(ds, 64, device="cuda", seed=seed, transform=tf)
        return [[x.cpu() for x, _ in loader] for _ in range(n)]

    (a0, a1), (b0,), (c0,) = epochs(2), epochs(1), epochs(1, seed=6)
    assert len(a0) == 4
    for x in a0:
        assert x.shape == (64, 3, 32, 32) and x.is_contiguous(memory_format=torch.channels_last)
    assert all(torch.equal(p, q) for p, q in zip(a0, b0))
    assert not all(torch.equal(p, q) for p, q in zip(a0, a1))
    assert not all(torch.equal(p, q) for p, q in zip(a0, c0))
