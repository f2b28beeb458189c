"""Stand-alone activations.

GELU, both of torch's forms (``approximate="none"``: erf; ``"tanh"``): CPU tensors run ``F.gelu``.
There is no gfx950 kernel for it yet: a GPU tensor raises instead of falling back to ATen, as
every op here does when its kernel is missing.

ReLU6, ``min(max(x, 0), 6)``, for a ReLU6 that follows no BatchNorm (``ops.batch_norm(relu6=True)``
fuses the one that does): on the GPU one forward kernel (csrc/elementwise.hip ``relu6_fwd``) that
also writes the backward's gate as one bit per element, and one backward kernel that reads dy and
that gate -- ``dx`` is exactly ``dy`` where ``0 < x < 6`` and exactly 0 elsewhere, both boundaries
included (torch's ``hardtanh_backward``). A NaN input stays NaN. CPU tensors run ``F.relu6``.

SiLU, ``x * sigmoid(x)`` (EfficientNet's activation): CPU tensors run ``F.silu``. Like GELU it has
no gfx950 kernel yet -- the kernel pair written for it was withheld together with the other
EfficientNet kernels (profiles/r19/efficientnet_b0.md) -- so a GPU tensor raises.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .._native import native


def gelu(x: torch.Tensor, approximate: str = "none") -> torch.Tensor:
    """``F.gelu(x, approximate=approximate)``."""
    if approximate not in ("none", "tanh"):
        raise ValueError(f"gelu: approximate must be 'none' or 'tanh', got {approximate!r}")
    if x.is_cuda:
        raise NotImplementedError("gelu has no native gfx950 kernel yet (CPU tensors only)")
    return F.gelu(x, approximate=approximate)


def _dense(x: torch.Tensor) -> bool:
    return x.is_contiguous() or (x.dim() == 4 and
                                 x.is_contiguous(memory_format=torch.channels_last))


class _ReLU6Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        if not _dense(x):
            x = x.contiguous()
        y, gate = native().relu6_fwd(x)
        ctx.save_for_backward(gate)
        ctx.strides = x.stride()
        return y

    @staticmethod
    def backward(ctx, dy):
        gate, = ctx.saved_tensors
        if dy.stride() != ctx.strides:
            # the gate is in the forward's memory order: bring dy into that layout
            dy = torch.empty_strided(dy.shape, ctx.strides, dtype=dy.dtype,
                                     device=dy.device).copy_(dy)
        return native().relu6_bwd(dy, gate)


def relu6(x: torch.Tensor) -> torch.Tensor:
    """``F.relu6(x)``."""
    if not x.is_cuda:
        return F.relu6(x)
    if x.dtype != torch.float32:
        raise TypeError(f"native relu6 expects float32, got {x.dtype}")
    return _ReLU6Fn.apply(x)


def silu(x: torch.Tensor) -> torch.Tensor:
    """``F.silu(x)``."""
    if x.is_cuda:
        raise NotImplementedError("silu has no native gfx950 kernel yet (CPU tensors only)")
    return F.silu(x)
