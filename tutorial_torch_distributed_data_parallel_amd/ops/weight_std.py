"""Weight standardisation (``csrc/weight_std.hip``): every output filter of a convolution weight
``[Cout, Cg, R, S]`` brought to zero mean and unit (biased) variance over its ``K = Cg*R*S``
elements,

    w_hat[o] = (w[o] - mean_K(w[o])) * rsqrt(var_K(w[o]) + eps)

with no affine gain (a model that wants one multiplies after the op). It is the companion of
GroupNorm in the recipes that train ResNets at small per-rank batches (Qiao et al., "Micro-Batch
Training with Batch-Channel Normalization and Weight Standardization"; Big Transfer).

On the GPU (float32 only; anything else raises ``TypeError``) the weight is read in place in
either memory layout a ``tdp.nn.Conv2d`` weight has -- channels_last ``[Cout][R][S][Cg]`` or the
stem's contiguous ``[Cout][Cg][R][S]``: in both, filter ``o`` is the dense run of ``K`` floats
at ``o*K``. Any other view raises ``ValueError``. ``w_hat`` has the weight's own strides, so
``ops.conv2d`` treats it exactly as it treats a parameter (no permute, no copy).

The backward reads the upstream gradient ``g = dL/dw_hat`` and ``w_hat`` (which the convolution
saves anyway; the weight itself is not needed) and writes

    dw[o] = rstd_o * (g[o] - mean_K(g[o]) - w_hat[o] * mean_K(g[o] * w_hat[o]))

straight into ``grad_dest(weight)``: the parameter's DDP gradient-arena slot when it has one.

CPU tensors run the torch composition under plain autograd: the oracle of the CPU tests and what
gloo DDP runs.
"""
from __future__ import annotations

import torch

from .._native import native
from ._grad import grad_dest


def _dense(w) -> bool:
    return w.is_contiguous() or w.is_contiguous(memory_format=torch.channels_last)


class _WeightStdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, eps):
        w_hat, rstd = native().ws_fwd(weight, eps)
        ctx.param = weight
        ctx.save_for_backward(w_hat, rstd)
        return w_hat

    @staticmethod
    def backward(ctx, g):
        w_hat, rstd = ctx.saved_tensors
        if g.stride() != w_hat.stride():  # the convolutions return w_hat's layout: not their path
            src, g = g, torch.empty_like(w_hat)
            native().copy4d(g, src)
        dw = grad_dest(ctx.param)
        if dw.stride() != w_hat.stride():
            raise ValueError("weight_standardize: the gradient slot does not have the weight's "
                             "memory layout")
        native().ws_bwd(g, w_hat, rstd, dw)
        return dw, None


def weight_standardize(weight: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """``(w - mean) * rsqrt(var + eps)`` per output filter of a ``[Cout, Cg, R, S]`` weight
    (biased variance over the filter's ``Cg*R*S`` elements). Always float32 arithmetic on the
    given (master) weight, inside ``tdp.autocast`` as outside it."""
    if weight.dim() != 4:
        raise ValueError(f"weight_standardize: expected a 4-D convolution weight "
                         f"(got {weight.dim()}-D)")
    eps = float(eps)
    if not weight.is_cuda:
        var, mean = torch.var_mean(weight, dim=(1, 2, 3), keepdim=True, unbiased=False)
        return (weight - mean) * torch.rsqrt(var + eps)
    if weight.dtype != torch.float32:
        raise TypeError(f"weight_standardize: the native kernels are float32 only "
                        f"(got {weight.dtype})")
    if weight.numel() == 0 or not _dense(weight):
        raise ValueError("weight_standardize: the weight must be a non-empty contiguous or "
                         "channels_last tensor (each filter one dense run of floats)")
    if not (torch.is_grad_enabled() and weight.requires_grad):
        return native().ws_fwd(weight.detach(), eps)[0]
    return _WeightStdFn.apply(weight, eps)
