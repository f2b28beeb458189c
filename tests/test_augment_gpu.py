"""tdp.data.augment_batch (csrc/image_augment.hip) against reference_augment, bit for bit: every
rule is integer or singly-rounded fp32, so no tolerance. Shapes: (37, 29, 3) has 3219 bytes per
sample, so later samples start unaligned; (32, 32, 3) is aligned; (70, 130, 3) spans several
tiles in both directions and three statistics chunks; (33, 47, 1) is one channel; (2, 5, 3) is the
Sharpness identity and mostly out of range for Affine. Every batch holds a random, a constant, a
two-valued and a single-outlier image (Equalize's step, AutoContrast's hi)."""
import pytest
import torch

from tutorial_torch_distributed_data_parallel_amd.data import (AugmentedTransform, CropTransform,
                                                               PrefetchLoader, TrivialAugment,
                                                               affine_params, augment_batch,
                                                               cifar_like_uint8,
                                                               reference_augment)
from tutorial_torch_distributed_data_parallel_amd.data import augment as A

pytestmark = pytest.mark.gpu
fb = A.float_bits

SHAPES = [(37, 29, 3), (32, 32, 3), (70, 130, 3), (33, 47, 1), (2, 5, 3)]
ROWS = ([[A.IDENTITY], [A.AUTOCONTRAST], [A.EQUALIZE]]
        + [[A.AFFINE] + affine_params(k, v) for k, v in
           [("shear_x", 0.99), ("shear_x", -0.99), ("shear_y", 0.99), ("shear_y", -0.99),
            ("rotate", 135), ("rotate", 45), ("rotate", 0), ("translate_x", 32),
            ("translate_x", -32), ("translate_y", 32), ("translate_y", -32),
            ("translate_x", 200)]]
        + [[op, fb(f)] for op in A._BLEND_OPS for f in (0.01, 1.0, 1.99)]
        + [[A.POSTERIZE, b] for b in (0, 2, 8)]
        + [[A.SOLARIZE, fb(t)] for t in (0.0, 128.5, 255.0)])


def images(shape, n=5):
    H, W, C = shape
    g = torch.Generator().manual_seed(H * W * C)
    x = torch.randint(0, 256, (n, H, W, C), dtype=torch.uint8, generator=g)
    x[1] = 93
    x[2] = torch.where(x[2] < 128, 17, 203).to(torch.uint8)
    x[3] = 100 + x[3] % 20
    x[3, H // 2, W // 2] = 255
    return x


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(str(v) for v in r))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_op_matches_reference(shape, row):
    x = images(shape)
    p = A.make_params([row] * len(x))
    assert torch.equal(augment_batch(x.cuda(), p).cpu(), reference_augment(x, p))


@pytest.mark.parametrize("f", [0.01, 1.99])
def test_contrast_gray_sum_past_2_24(f):
    x = torch.full((1, 300, 300, 3), 255, dtype=torch.uint8)  # sum of gray = 254 * 90000
    p = A.make_params([[A.CONTRAST, fb(f)]])
    assert torch.equal(augment_batch(x.cuda(), p).cpu(), reference_augment(x, p))


@pytest.mark.parametrize("shape", [(37, 29, 3), (70, 130, 3)], ids=str)
def test_mixed_batch(shape):
    x = images(shape, len(ROWS))
    p = A.make_params(ROWS)
    xc = x.cuda()
    out = augment_batch(xc, p)
    assert torch.equal(out, augment_batch(xc, p))
    assert torch.equal(out.cpu(), reference_augment(x, p))
    for n in range(len(ROWS)):  # sample n depends on sample n alone
        assert torch.equal(augment_batch(xc[n:n + 1].clone(), p[n:n + 1]), out[n:n + 1]), n
    # a view that starts 1 byte into its storage: no 16-byte units, the same result
    store = torch.empty(x.numel() + 1, dtype=torch.uint8, device="cuda")
    store[1:].copy_(xc.view(-1))
    assert torch.equal(augment_batch(store[1:].view(x.shape), p), out)
    # device params are not read back: an op outside the table is Identity
    bad = p.clone()
    bad[::2, 0], bad[1::2, 0] = 99, -1
    assert torch.equal(augment_batch(xc, bad.cuda()), xc)


def test_graph_replays_match_eager():
    shape = (70, 130, 3)
    xs = images(shape, len(ROWS)).cuda()
    ps = A.make_params(ROWS).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        augment_batch(xs, ps)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = augment_batch(xs, ps)
    for k in range(3):
        g = torch.Generator().manual_seed(k)
        x = torch.randint(0, 256, xs.shape, dtype=torch.uint8, generator=g).cuda()
        p = A.make_params(ROWS)[torch.randperm(len(ROWS), generator=g)].cuda()
        xs.copy_(x)
        ps.copy_(p)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, augment_batch(x, p)), k


def test_prefetch_loader_end_to_end():
    from test_crop_resize_gpu import tolerance

    ds = cifar_like_uint8(n=256)

    def batches(device):
        tf = AugmentedTransform(TrivialAugment(), CropTransform(
            size=32, crop="random_pad", padding=4, mean=[0.0] * 3, std=[1 / 255] * 3,
            round_u8=False))
        return [x.cpu() for x, _ in PrefetchLoader(ds, 64, device=device, seed=3, transform=tf)]

    gpu, cpu = batches("cuda"), batches("cpu")
    assert len(gpu) == len(cpu) == 4
    tol = tolerance(torch.tensor([[0, 0, 32, 32]]), (32, 32))
    for a, b in zip(gpu, cpu):
        assert (a - b).abs().max().item() <= tol
