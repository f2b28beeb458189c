"""The uint8 form of image_crop_resize (csrc/image_crop.hip) and image_normalize_erase
(csrc/image_finish.hip) against the float crop (bitwise), reference_normalize_erase (bitwise in the
constant modes) and, for value="random", the float64 rule of tests/test_mix_gpu.py."""
import pytest
import torch

from test_crop_resize_gpu import oracle, tolerance
from tutorial_torch_distributed_data_parallel_amd.data import (CropTransform, RandomErasing,
                                                               TrivialAugment, crop_resize,
                                                               normalize_erase,
                                                               reference_normalize_erase)
from tutorial_torch_distributed_data_parallel_amd.data import erase as E
from tutorial_torch_distributed_data_parallel_amd.data.host import reference_crop_resize

pytestmark = pytest.mark.gpu
MEAN, STD = (0.4914, 0.4822, 0.4465, 0.5), (0.2023, 0.1994, 0.2010, 0.25)
LAYOUTS = [True, False]


def _images(shape, seed=0):
    return torch.randint(0, 256, shape, dtype=torch.uint8,
                         generator=torch.Generator().manual_seed(seed))


# (H, W, C, size): (200, 37, 4, 7) takes several chunks of the LDS stage, (32, 32, 3, 32) is the
# identity resize
@pytest.mark.parametrize("H,W,C,size", [(9, 11, 3, 5), (40, 33, 1, 16), (200, 37, 4, 7),
                                        (32, 32, 3, 32)])
def test_uint8_crop_is_the_float_crop(H, W, C, size):
    x = _images((4, H, W, C), seed=H)
    boxes = torch.tensor([(0, 0, H, W), (-2, -3, H, W), (1, 2, H - 2, W - 3), (H // 2, W // 2, H, W)],
                         dtype=torch.int32)
    if size == H:
        boxes[1:] = boxes[0]  # the identity resize stays one
    flip = torch.tensor([1, 0, 1, 0], dtype=torch.uint8)
    mean, std = MEAN[:C], STD[:C]
    xc, fc = x.cuda(), flip.cuda()
    u8 = crop_resize(xc, boxes, fc, size, mean, std, out_dtype=torch.uint8)
    assert u8.dtype == torch.uint8 and u8.shape == (4, size, size, C) and u8.is_contiguous()
    for cl in LAYOUTS:
        want = crop_resize(xc, boxes, fc, size, mean, std, channels_last=cl)
        got = normalize_erase(u8, mean, std, channels_last=cl)
        assert got.stride() == want.stride() and torch.equal(got, want), cl
    # the rounded value is the float64 oracle's wherever the unrounded value, which the kernel holds
    # to `tolerance`, is further than that from a rounding boundary; reference_crop_resize, itself
    # fp32, gets the same allowance again
    ref = oracle(x, boxes, flip, (size, size))
    margin, tol = ((ref - ref.floor()) - 0.5).abs(), tolerance(boxes, (size, size))
    got = u8.cpu().permute(0, 3, 1, 2)
    assert (margin > tol).double().mean() > 0.9
    assert torch.equal(got.double()[margin > tol], ref.round()[margin > tol])
    ref32 = reference_crop_resize(x, boxes, flip, (size, size), mean, std, out_dtype=torch.uint8)
    assert torch.equal(got[margin > 2 * tol], ref32.permute(0, 3, 1, 2)[margin > 2 * tol])
    if size == H:
        assert torch.equal(u8.cpu(), torch.where(flip.bool().view(-1, 1, 1, 1), x.flip(2), x))


def _erase_boxes(H, W):
    # one pixel, touching the last row and column, the whole image, none
    return torch.tensor([(H // 2, W // 3, 1, 1), (H - 3, W - 2, 3, 2), (0, 0, H, W), (1, 1, 0, 5)],
                        dtype=torch.int32)


# W C is a multiple of 16 at W = 16, and not at W = 13; 150 x 31 is several strips and segments
@pytest.mark.parametrize("H,W,offset", [(6, 16, 0), (6, 16, 1), (7, 13, 0), (7, 13, 1),
                                        (150, 31, 0)])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("cl", LAYOUTS)
def test_erase_constant_is_the_reference(cl, C, H, W, offset):
    n = 4 * H * W * C
    x = _images((n + offset,), seed=C * W).cuda()[offset:].view(4, H, W, C)  # 1 byte into its storage
    assert x.data_ptr() % 16 == offset and x.is_contiguous()
    boxes, mean, std = _erase_boxes(H, W), MEAN[:C], STD[:C]
    for value in (0.0, -0.75, tuple(0.5 * c - 1.0 for c in range(C))):
        for b in (boxes, boxes.cuda()):
            got = normalize_erase(x, mean, std, b, value, channels_last=cl)
            assert torch.equal(got, reference_normalize_erase(x, mean, std, boxes, value))
    out_of_image = torch.tensor([(-2, -3, 5, 6), (H - 1, W - 1, 9, 9), (0, 0, 0, 0), (3, 2, 2, 2)],
                                dtype=torch.int32)  # device boxes are clamped by the kernel
    got = normalize_erase(x, mean, std, out_of_image.cuda(), 2.0, channels_last=cl)
    assert torch.equal(got, reference_normalize_erase(x, mean, std, out_of_image, 2.0))


@pytest.mark.parametrize("H,W,C", [(12, 16, 3), (9, 13, 4), (150, 31, 1)])
def test_erase_random(H, W, C):
    x = _images((4, H, W, C), seed=5).cuda()
    boxes, mean, std = _erase_boxes(H, W), MEAN[:C], STD[:C]
    seed = (0x9E3779B9 << 32) | 12345
    out = {cl: normalize_erase(x, mean, std, boxes, "random", seed, channels_last=cl)
           for cl in LAYOUTS}
    assert torch.equal(out[True], out[False])
    assert torch.equal(out[True], normalize_erase(x, mean, std, boxes, "random", seed))
    inside = reference_normalize_erase(x, mean, std, boxes, 7.0) == 7.0
    assert torch.equal(out[True][~inside], reference_normalize_erase(x, mean, std)[~inside])
    u1, u2 = E.philox_uniforms(seed, 4, C, H, W, device="cuda")
    z64 = E.normal_from_uniforms(u1, u2, torch.float64)[inside]
    e_k = (out[True][inside].double() - z64).abs().max().item()
    e_t = (E.normal_from_uniforms(u1, u2, torch.float32)[inside].double() - z64).abs().max().item()
    needed = (e_k - 4 * e_t) / (2.0 ** -24 * z64.abs().max().item())
    print(f"[rule] erase random {H}x{W}x{C}: e_k={e_k:.3e} e_t={e_t:.3e} needed c={needed:.3f}")
    assert e_k <= 4 * e_t + 2 * 2.0 ** -24 * z64.abs().max().item()
    assert abs(z64.mean().item()) < 0.2 and abs(z64.std().item() - 1) < 0.2  # whole-image box
    # sample 2 alone, told that it is sample 2, is the batch's sample 2; another seed is not
    alone = normalize_erase(x[2:3], mean, std, boxes[2:3], "random", seed, sample_offset=2)
    assert torch.equal(alone[0], out[True][2])
    other = normalize_erase(x, mean, std, boxes, "random", seed + 1)
    assert not torch.equal(other[2], out[True][2])
    assert torch.equal(other[~inside], out[True][~inside])


def test_errors():
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8).cuda()
    m, s = MEAN[:3], STD[:3]
    with pytest.raises(TypeError):
        normalize_erase(x.float(), m, s)
    with pytest.raises(ValueError):
        normalize_erase(x[..., :2].contiguous(), m[:2], s[:2])
    for bad in ([(0, 0, 9, 4), (0, 0, 0, 0)], [(0, 0, 0, 0), (-1, 0, 3, 3)], [(0, 6, 2, 3)] * 2):
        with pytest.raises(ValueError):
            normalize_erase(x, m, s, torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(ValueError):
        crop_resize(x, torch.tensor([(0, 0, 8, 8)] * 2, dtype=torch.int32), None, 4, m, s,
                    round_u8=False, out_dtype=torch.uint8)


def test_graph_replays_match_eager():
    tf = CropTransform(size=24, augment=TrivialAugment(), erase=RandomErasing(p=1.0, value="random"))
    ta, er = TrivialAugment(), RandomErasing(p=1.0)

    def draw(k):  # every parameter as a device tensor: nothing is validated or read back
        g = torch.Generator().manual_seed(k)
        ta.start_epoch(k)
        er.start_epoch(k)
        return [_images((4, 40, 40, 3), seed=k).cuda(),
                torch.randint(0, 2, (4,), dtype=torch.uint8, generator=g).cuda(),
                tf.boxes(4, 40, 40).cuda(), ta.draw(4, 24, 24).cuda(), er.draw(4, 24, 24)[0].cuda()]

    static = draw(100)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tf.apply(*static, seed=77)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = tf.apply(*static, seed=77)
    for k in range(3):
        fresh = draw(k)
        for dst, src in zip(static, fresh):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, tf.apply(*fresh, seed=77)), k
