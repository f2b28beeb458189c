"""tdp.nn.MultiheadAttention on CPU tensors (the plain torch composition) against
torch.nn.MultiheadAttention, and the refusals of the attention ops."""
import pytest
import torch

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops


@pytest.mark.parametrize("E, H, bias", [(64, 2, True), (128, 2, True), (64, 2, False)])
def test_module_matches_torch_and_state_dicts_load_both_ways(E, H, bias):
    torch.manual_seed(0)
    ours = tdp.nn.MultiheadAttention(E, H, bias=bias)
    twin = torch.nn.MultiheadAttention(E, H, bias=bias, batch_first=True)
    with torch.no_grad():
        for n, p in twin.named_parameters():
            if n.endswith("bias"):  # torch initialises them to zero
                p.uniform_(-0.1, 0.1)
    ours.load_state_dict(twin.state_dict())
    back = torch.nn.MultiheadAttention(E, H, bias=bias, batch_first=True)
    back.load_state_dict(ours.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(back.parameters(), twin.parameters()))
    x = torch.randn(2, 5, E)
    xo, xt = x.clone().requires_grad_(), x.clone().requires_grad_()
    y, w = ours(xo)
    yt, _ = twin(xt, xt, xt, need_weights=False)
    assert w is None
    g = torch.randn_like(yt)
    y.backward(g)
    yt.backward(g)
    torch.testing.assert_close(y, yt)
    torch.testing.assert_close(xo.grad, xt.grad)
    names = [n for n, _ in twin.named_parameters()]
    assert names == [n for n, _ in ours.named_parameters()]
    for n, p, q in zip(names, ours.parameters(), twin.parameters()):
        torch.testing.assert_close(p.grad, q.grad, msg=lambda s: f"{n}: {s}")


@pytest.mark.parametrize("kw", [dict(attn_mask=torch.ones(5, 5)), dict(is_causal=True),
                                dict(dropout_p=0.1)])
def test_op_refuses(kw):
    q = torch.randn(1, 1, 5, 32)
    with pytest.raises(NotImplementedError):
        ops.scaled_dot_product_attention(q, q, q, **kw)


@pytest.mark.parametrize("kw", [dict(batch_first=False), dict(kdim=32), dict(vdim=32),
                                dict(dropout=0.1)])
def test_module_refuses_at_construction(kw):
    with pytest.raises(NotImplementedError):
        tdp.nn.MultiheadAttention(64, 2, **kw)


def test_module_refuses_other_head_sizes_naming_the_supported_ones():
    with pytest.raises(NotImplementedError, match="32 and 64"):
        tdp.nn.MultiheadAttention(64, 4)


def test_module_refuses_at_call():
    m = tdp.nn.MultiheadAttention(64, 2)
    x = torch.randn(2, 5, 64)
    for kw in (dict(need_weights=True), dict(attn_mask=torch.ones(5, 5)), dict(is_causal=True),
               dict(key=torch.randn(2, 3, 64)), dict(key_padding_mask=torch.zeros(2, 5))):
        with pytest.raises(NotImplementedError):
            m(x, **kw)
