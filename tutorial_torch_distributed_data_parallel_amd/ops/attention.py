"""Fused attention (``csrc/attention.hip``): ``softmax(scale * q k^T) v`` per (batch, head).

One forward kernel chains both GEMMs through an online softmax in registers; the backward is a
``rowsum(dO * o)`` pass, a dq kernel and a dk / dv kernel that recompute the probabilities from the
saved per-query log-sum-exp. The ``[B, H, S, S]`` score matrix is never written in either
direction; the output and ``lse`` are all that is saved beside the inputs. Every GEMM of the op is
an fp32 GEMM on the bf16 matrix core (exact three-way split, six kept products, fp32 accumulation),
softmax statistics are fp32, there are no atomics, and the work partition depends on
``(Sq, Sk, D)`` only: two runs agree bitwise and a sample does not see the batch around it.

GPU tensors are float32 with head size 32 or 64; anything else raises (``TypeError`` for a dtype,
``NotImplementedError`` for a head size, ``ValueError`` for ``B * H > 65535``). There are no masks,
no causal form and no dropout. Operands are read in place through their strides when the last
dimension has stride 1 and every row is 16-byte aligned (a packed ``[B, S, 3E]`` projection is);
any other view gets one native strided copy (``attn_copy4d``). The output's memory is
``[B, Sq, H, D]``, so ``out.transpose(1, 2).reshape(B, Sq, H * D)`` is a view.

Inside ``tdp.autocast`` the attention core stays on this fp32 form, bitwise equal to outside the
region: only the projections around it (``ops.linear``) change precision. A single-product bf16
form of the core is a follow-up.

CPU tensors run the plain torch composition in fp32 under plain autograd.
"""
from __future__ import annotations

import torch

from .._native import native

HEAD_SIZES = (32, 64)


def _composition(q, k, v, scale):
    return torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v


def _readable(t: torch.Tensor) -> torch.Tensor:
    """``t`` ([B, H, S, D]) as the kernels read it: in place, or one native strided copy."""
    if t.stride(3) == 1 and all(s % 4 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0:
        return t
    return native().attn_copy4d(t)


def _check(q, k, v):
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype != torch.float32:
            raise TypeError(f"attention: the native kernels are float32 only ({name} is {t.dtype})")
    if q.dim() != 4 or k.dim() != 4 or v.shape != k.shape or q.shape[:2] != k.shape[:2] or \
            q.shape[3] != k.shape[3]:
        raise ValueError("attention: q must be [B, H, Sq, D] and k, v [B, H, Sk, D] "
                         f"(got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)})")
    B, H, Sq, D = q.shape
    if D not in HEAD_SIZES:
        raise NotImplementedError(f"attention: head size {D} has no kernel; the supported head "
                                  f"sizes are {HEAD_SIZES[0]} and {HEAD_SIZES[1]}")
    if B * H > 65535:
        raise ValueError(f"attention: B * H = {B * H} exceeds 65535")
    if q.numel() == 0 or k.numel() == 0:
        raise ValueError("attention: empty input")


def _backward(ctx, dout, dq, dk, dv):
    q, k, v, o, lse = ctx.saved_tensors
    native().attn_bwd(_readable(dout), q, k, v, o, lse, ctx.scale, dq, dk, dv)


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        q, k, v = _readable(q), _readable(k), _readable(v)
        o, lse = native().attn_fwd(q, k, v, scale)
        ctx.scale = scale
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k = ctx.saved_tensors[:2]
        B, H, Sq, D = q.shape
        Sk = k.shape[2]
        dq = torch.empty((B, Sq, H, D), device=q.device, dtype=q.dtype).transpose(1, 2)
        dkv = torch.empty((2, B, Sk, H, D), device=q.device, dtype=q.dtype).transpose(2, 3)
        _backward(ctx, dout, dq, dkv[0], dkv[1])
        return dq, dkv[0], dkv[1], None


def _unpack(qkv, num_heads):
    """[B, S, 3E] -> q, k, v as [B, H, S, D] views."""
    D = qkv.shape[2] // (3 * num_heads)
    return qkv.unflatten(2, (3, num_heads, D)).permute(2, 0, 3, 1, 4).unbind(0)


class _PackedAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, num_heads, scale):
        q, k, v = _unpack(qkv, num_heads)
        o, lse = native().attn_fwd(q, k, v, scale)
        ctx.scale, ctx.num_heads = scale, num_heads
        ctx.save_for_backward(q, k, v, o, lse)
        B, S = qkv.shape[:2]
        return o.transpose(1, 2).reshape(B, S, -1)  # a view: o's memory is [B, S, H, D]

    @staticmethod
    def backward(ctx, dy):
        q = ctx.saved_tensors[0]
        B, H, S, D = q.shape
        dqkv = torch.empty((B, S, 3 * H * D), device=q.device, dtype=q.dtype)
        dq, dk, dv = _unpack(dqkv, H)
        dout = dy.view(B, S, H, D).transpose(1, 2)  # splitting a dimension is always a view
        _backward(ctx, dout, dq, dk, dv)
        return dqkv, None, None


def scaled_dot_product_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                 scale: float | None = None, *, attn_mask=None,
                                 dropout_p: float = 0.0, is_causal: bool = False) -> torch.Tensor:
    """``softmax(scale * q @ k.transpose(-1, -2)) @ v`` for q ``[B, H, Sq, D]`` and k, v
    ``[B, H, Sk, D]``; ``scale`` defaults to ``D ** -0.5``. Differentiable in q, k and v. Masks,
    the causal form and dropout raise ``NotImplementedError``. Computes in float32 inside
    ``autocast`` as outside it (bitwise the same result); a bf16 form is a follow-up."""
    if attn_mask is not None or is_causal or dropout_p > 0:
        raise NotImplementedError("attention: attn_mask, is_causal and dropout_p > 0 have no "
                                  "kernel")
    scale = float(q.shape[-1] ** -0.5 if scale is None else scale)
    if not q.is_cuda:
        return _composition(q, k, v, scale)
    _check(q, k, v)
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))):
        return native().attn_fwd(_readable(q.detach()), _readable(k.detach()),
                                 _readable(v.detach()), scale)[0]
    return _AttentionFn.apply(q, k, v, scale)


def attention_qkvpacked(qkv: torch.Tensor, num_heads: int,
                        scale: float | None = None) -> torch.Tensor:
    """Self-attention on a packed projection: ``qkv`` is ``[B, S, 3 * E]`` (q | k | v along the
    last dimension, each ``num_heads`` heads of ``E / num_heads``), read in place through strides;
    returns ``[B, S, E]``. The backward writes dq, dk and dv straight into one contiguous
    ``[B, S, 3 * E]`` gradient. The same kernels as ``scaled_dot_product_attention``; float32
    inside ``autocast`` as outside it (a bf16 form is a follow-up)."""
    num_heads = int(num_heads)
    if qkv.dim() != 3 or num_heads < 1 or qkv.shape[2] % (3 * num_heads):
        raise ValueError(f"attention_qkvpacked: expected [B, S, 3 * E] with E divisible by "
                         f"{num_heads} heads (got {tuple(qkv.shape)})")
    D = qkv.shape[2] // (3 * num_heads)
    scale = float(D ** -0.5 if scale is None else scale)
    if not qkv.is_cuda:
        q, k, v = _unpack(qkv, num_heads)
        B, S = qkv.shape[:2]
        return _composition(q, k, v, scale).transpose(1, 2).reshape(B, S, -1)
    q, k, v = _unpack(qkv.detach(), num_heads)
    _check(q, k, v)
    if not qkv.is_contiguous() or qkv.data_ptr() % 16:
        q, k, v = _unpack(qkv, num_heads)  # a view the kernels cannot read in place
        o = scaled_dot_product_attention(q, k, v, scale=scale)
        return o.transpose(1, 2).reshape(qkv.shape[0], qkv.shape[1], -1)
    if not (torch.is_grad_enabled() and qkv.requires_grad):
        B, S = qkv.shape[:2]
        return native().attn_fwd(q, k, v, scale)[0].transpose(1, 2).reshape(B, S, -1)
    return _PackedAttentionFn.apply(qkv, num_heads, scale)
