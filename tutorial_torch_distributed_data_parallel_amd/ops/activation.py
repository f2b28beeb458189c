"""GELU, both of torch's forms (``approximate="none"``: erf; ``"tanh"``).

CPU tensors run ``F.gelu``. There is no gfx950 kernel for it yet: a GPU tensor raises instead of
falling back to ATen, as every op here does when its kernel is missing.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def gelu(x: torch.Tensor, approximate: str = "none") -> torch.Tensor:
    """``F.gelu(x, approximate=approximate)``."""
    if approximate not in ("none", "tanh"):
        raise ValueError(f"gelu: approximate must be 'none' or 'tanh', got {approximate!r}")
    if x.is_cuda:
        raise NotImplementedError("gelu has no native gfx950 kernel yet (CPU tensors only)")
    return F.gelu(x, approximate=approximate)
