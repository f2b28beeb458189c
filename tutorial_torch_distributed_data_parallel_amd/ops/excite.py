"""Squeeze-and-excitation gate and stochastic depth.

``se_scale(x, t)``: ``y[n, c, h, w] = x[n, c, h, w] * sigmoid(t[n, c])`` for ``t`` of shape
``[N, C]`` or ``[N, C, 1, 1]``. CPU tensors run torch ops. There is no gfx950 kernel for it yet --
the forward / backward pair written for it (16-byte accesses along C, a fixed-order reduction for
``dt``) was withheld together with the other EfficientNet kernels
(profiles/r19/efficientnet_b0.md) -- so a GPU tensor raises, as every op here does when its
kernel is missing.

``stochastic_depth(x, p, training)``: torchvision's ``"row"`` mode. The per-sample keep mask --
Bernoulli(1 - p) scaled by 1 / (1 - p) -- is drawn with torch's generator as an ``[N]`` tensor on
``x``'s device; on the GPU one native kernel (csrc/excite.hip ``sample_scale``) applies it per
sample, and the same kernel applies it to ``dy``. ``p == 0`` or eval returns ``x`` itself,
``p == 1`` returns zeros. ``"batch"`` mode is not implemented.
"""
from __future__ import annotations

import torch

from .._native import native

_CL = torch.channels_last


def se_scale(x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """``x * sigmoid(t)[:, :, None, None]`` for ``x`` [N, C, H, W] and ``t`` [N, C] or
    [N, C, 1, 1]."""
    if x.dim() != 4 or t.shape[:2] != x.shape[:2] or t.numel() != x.shape[0] * x.shape[1]:
        raise ValueError(f"se_scale: x [N, C, H, W] and t [N, C] or [N, C, 1, 1] expected, got "
                         f"{tuple(x.shape)} and {tuple(t.shape)}")
    if x.is_cuda:
        raise NotImplementedError("se_scale has no native gfx950 kernel yet (CPU tensors only)")
    return x * torch.sigmoid(t).reshape(x.shape[0], x.shape[1], 1, 1)


def _dense(x):
    return x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=_CL))


class _SampleScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        if not _dense(x):
            x = x.contiguous()
        ctx.save_for_backward(scale)
        return native().sample_scale(x, scale)

    @staticmethod
    def backward(ctx, dy):
        scale, = ctx.saved_tensors
        if not _dense(dy):  # either dense layout keeps a sample's elements together
            dy = dy.contiguous()
        return native().sample_scale(dy, scale), None


def stochastic_depth(x: torch.Tensor, p: float, training: bool = True, generator=None,
                     mode: str = "row") -> torch.Tensor:
    """torchvision's ``stochastic_depth(x, p, "row", training)``: each sample of the batch is
    zeroed with probability ``p`` and scaled by ``1 / (1 - p)`` otherwise."""
    if mode != "row":
        raise NotImplementedError(f"stochastic_depth: only mode='row' is supported, got {mode!r}")
    if p < 0.0 or p > 1.0:
        raise ValueError(f"stochastic_depth: p must be in [0, 1], got {p}")
    if not training or p == 0.0:
        return x
    if p == 1.0:
        return torch.zeros_like(x)
    keep = 1.0 - p
    scale = torch.empty(x.shape[0], dtype=x.dtype, device=x.device)
    scale.bernoulli_(keep, generator=generator).div_(keep)
    if not x.is_cuda:
        return x * scale.view((-1,) + (1,) * (x.dim() - 1))
    if x.dtype != torch.float32:
        raise TypeError(f"native stochastic_depth expects float32, got {x.dtype}")
    return _SampleScaleFn.apply(x, scale)
