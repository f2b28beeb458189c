"""tdp.data.mix_batch (csrc/mix.hip) against the float64 composition: pure-copy elements (inside
a box, or outside it with lam == 1) bitwise the source, mixed elements by the rule of
tests/test_hard_inputs_gpu.py with c = 2 and scale = max|x| (e_t: the fp32 composition on the GPU).
(3, 5, 7) has 105 floats per sample -- the 4-byte form; (4, 6, 6) and (8, 4, 5) take 16-byte
units, which in the contiguous layout cross row ends and box edges."""
import pytest
import torch

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.data.mix import reference_mix

pytestmark = pytest.mark.gpu

CASES = [((3, 5, 7), False), ((3, 5, 7), True), ((4, 6, 6), False), ((4, 6, 6), True),
         ((8, 4, 5), True)]


@pytest.mark.parametrize("perm_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("chw,channels_last", CASES)
def test_mix_batch(chw, channels_last, perm_dtype):
    C, H, W = chw
    x = torch.randn(3, C, H, W, generator=torch.Generator().manual_seed(C * H * W)).cuda()
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    perm = torch.tensor([1, 0, 2], dtype=perm_dtype).cuda()  # a fixed point at 2
    lam = torch.tensor([0.3, 1.0, 0.6]).cuda()
    # an empty box (MixUp) | clipped by the top and the right edge (CutMix) | the whole image
    boxes = torch.tensor([[1, 1, 0, 0], [-2, W - 3, 4, 9], [0, 0, H, W]], dtype=torch.int32).cuda()
    out = tdp.data.mix_batch(x, perm, lam, boxes)
    assert out.stride() == x.stride()
    assert torch.equal(out, tdp.data.mix_batch(x, perm, lam, boxes))
    ref = reference_mix(x.double().cpu(), perm.cpu(), lam.cpu(), boxes.cpu())
    t32 = reference_mix(x, perm, lam, boxes)
    inside = torch.zeros(3, 1, H, W, dtype=torch.bool)
    inside[1, :, 0:2, W - 3:] = True
    inside[2] = True
    copy = (inside | (lam.cpu() == 1).view(3, 1, 1, 1)).expand_as(ref)
    assert torch.equal(out.cpu()[copy].double(), ref[copy])
    e_k = (out.double().cpu() - ref).abs().max().item()
    e_t = (t32.double().cpu() - ref).abs().max().item()
    print(f"[rule] mix{chw}: e_k={e_k:.3e} e_t={e_t:.3e}")
    assert e_k <= 4 * e_t + 2 * 2.0 ** -24 * x.abs().max().item()


def test_refuses_grad():
    x = torch.randn(2, 3, 4, 4, device="cuda", requires_grad=True)
    with pytest.raises(ValueError):
        tdp.data.mix_batch(x, torch.tensor([1, 0]).cuda(), torch.ones(2).cuda(),
                           torch.zeros(2, 4, dtype=torch.int32).cuda())
