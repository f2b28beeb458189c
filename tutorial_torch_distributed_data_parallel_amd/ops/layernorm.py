"""Layer norm over the last dimension(s) of a float32 tensor.

CPU tensors run ``F.layer_norm`` (what the gloo and unit tests exercise). There is no gfx950
kernel for it yet: a GPU tensor raises instead of falling back to ATen, as every op here does
when its kernel is missing. ``note_use`` is called for the affine parameters in forward, so a
LayerNorm applied twice in one forward is counted like any other reused DDP parameter.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._grad import note_use


def layer_norm(x: torch.Tensor, normalized_shape, weight: torch.Tensor | None = None,
               bias: torch.Tensor | None = None, eps: float = 1e-5) -> torch.Tensor:
    """``F.layer_norm(x, normalized_shape, weight, bias, eps)``."""
    if isinstance(normalized_shape, int):
        normalized_shape = (normalized_shape,)
    normalized_shape = tuple(int(d) for d in normalized_shape)
    nd = len(normalized_shape)
    if nd == 0 or tuple(x.shape[-nd:]) != normalized_shape:
        raise ValueError(f"layer_norm: input shape {tuple(x.shape)} does not end in "
                         f"normalized_shape {normalized_shape}")
    if x.is_cuda:
        raise NotImplementedError("layer_norm has no native gfx950 kernel yet (CPU tensors only)")
    if torch.is_grad_enabled():
        note_use(weight)
        note_use(bias)
    return F.layer_norm(x, normalized_shape, weight, bias, eps)
