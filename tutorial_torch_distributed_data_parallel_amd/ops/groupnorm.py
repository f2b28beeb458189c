"""Group norm (``csrc/groupnorm.hip``): ``act(group_norm(x) [+ residual])`` with act none or ReLU.

Statistics are per (sample, group), so there is no collective, no running statistic and no
difference between training and eval: the result for a sample does not depend on the batch around
it (bitwise, on the GPU kernels), which is what makes it the alternative to SyncBatchNorm when the
per-rank batch is small.

Layout forms on the GPU (float32 only; anything else raises ``TypeError``):
  NHWC    -- a 4-D channels_last input with ``C % 4 == 0`` (16-byte aligned): what the
             implicit-GEMM convolutions produce. The output is channels_last.
  generic -- everything else, on ``x.contiguous()``: NCHW with any C, 3-D ``[N, C, L]``,
             2-D ``[N, C]``, views at any storage offset.

The ReLU gate of the backward (``y > 0``, zero gradient at 0, as the BatchNorm kernels): the NHWC
form saves BatchNorm's 1-byte-per-4-channels mask, written by the normalisation pass, and never
the float output; the generic form saves the output ``y`` and gates on ``y > 0``. Without a ReLU
neither is saved: the backward needs only x, the weight and the [mean | rstd] statistics.

``dw`` / ``db`` are written straight into ``grad_dest(param)`` (the DDP gradient arena slot), as
``_BatchNormFn`` does; there is no in-place optimizer epilogue. ``residual_grad_into`` (a
``SharedGrad``) receives the gradient of the fused residual, the ReLU-masked ``dy``.

CPU tensors run ``F.group_norm`` (+ residual, + ``F.relu``) under plain autograd: the oracle of the
CPU tests and what gloo DDP runs.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .._native import native
from ._grad import grad_dest, needs


def _nhwc_form(x) -> bool:
    return x.dim() == 4 and x.shape[1] % 4 == 0 and \
        x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0


def _rows3(x):
    """[N, C, H, W] channels_last -> its memory as [N, HW, C]."""
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])


def _unrows3(y3, shape4):
    N, C, H, W = shape4
    return y3.view(N, H, W, C).permute(0, 3, 1, 2)


def _to_form(t, nhwc):
    """``t`` ([N, C, *]) in the memory form the kernels take."""
    if nhwc:
        return _rows3(t.contiguous(memory_format=torch.channels_last))
    return t.contiguous()


class _GroupNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, relu, residual, sink):
        nhwc = _nhwc_form(x)
        shape = tuple(x.shape)
        xm = _to_form(x, nhwc)
        rm = _to_form(residual, nhwc) if residual is not None else None
        if nhwc and rm is not None and rm.data_ptr() % 16:
            rm = rm.clone()
        out = native().gn_fwd(xm, groups, weight, bias, float(eps), relu=relu, residual=rm,
                              nhwc=nhwc, want_mask=bool(relu and nhwc))
        y, stats = out[0], out[1]
        mask = out[2] if len(out) > 2 else None
        ctx.nhwc, ctx.shape, ctx.groups = nhwc, shape, groups
        ctx.params = (weight, bias)
        ctx.has_res = residual is not None
        ctx.sink = sink
        ctx.save_for_backward(xm, weight, stats, y if (relu and not nhwc) else None, mask)
        return _unrows3(y, shape) if nhwc else y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        xm, weight, stats, y, mask = ctx.saved_tensors
        nhwc = ctx.nhwc
        dym = _to_form(dy, nhwc).reshape(xm.shape)
        if nhwc and dym.data_ptr() % 16:
            dym = dym.clone()
        w_param, b_param = ctx.params
        dw = grad_dest(w_param) if (w_param is not None and needs(ctx, 1)) else None
        db = grad_dest(b_param) if (b_param is not None and needs(ctx, 2)) else None
        want_res = ctx.has_res and needs(ctx, 6)
        dx, dres, dw, db = native().gn_bwd(dym, xm, stats, ctx.groups, weight, y_relu=y,
                                           mask=mask, nhwc=nhwc, want_dx=needs(ctx, 0),
                                           want_dres=want_res, dw=dw, db=db)
        if nhwc:
            dx = _unrows3(dx, ctx.shape) if dx is not None else None
            dres = _unrows3(dres, ctx.shape) if dres is not None else None
        else:
            dx = dx.view(ctx.shape) if dx is not None else None
            dres = dres.view(ctx.shape) if dres is not None else None
        if dres is not None and ctx.sink is not None:
            dres = ctx.sink.deposit(dres)  # the forked block input's shared gradient
        return dx, dw, db, None, None, None, dres, None


def group_norm(x: torch.Tensor, num_groups: int, weight: torch.Tensor | None = None,
               bias: torch.Tensor | None = None, eps: float = 1e-5, relu: bool = False,
               residual: torch.Tensor | None = None, residual_grad_into=None) -> torch.Tensor:
    """``relu?(F.group_norm(x, num_groups, weight, bias, eps) [+ residual])`` over dim 1 of x
    ([N, C] or [N, C, *]). Training and eval are the same computation. The op computes in float32
    inside ``autocast`` as outside it (bitwise the same result)."""
    if x.dim() < 2:
        raise ValueError(f"group_norm: expected at least 2D input (got {x.dim()}D input)")
    num_groups = int(num_groups)
    C = x.shape[1]
    if num_groups < 1 or C % num_groups:
        raise ValueError(f"group_norm: {C} channels are not divisible into {num_groups} groups")
    if residual is not None and residual.shape != x.shape:
        raise ValueError("group_norm: residual must have the input's shape")
    relu = bool(relu)
    if not x.is_cuda:
        y = F.group_norm(x, num_groups, weight, bias, eps)
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y
    for t in (x, weight, bias, residual):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"group_norm: the native kernels are float32 only (got {t.dtype})")
    if x.numel() == 0:
        raise ValueError("group_norm: empty input")
    if not (torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in (x, weight, bias, residual))):
        # nothing to differentiate: the same kernels, nothing saved (no mask either)
        nhwc = _nhwc_form(x)
        rm = _to_form(residual.detach(), nhwc) if residual is not None else None
        if nhwc and rm is not None and rm.data_ptr() % 16:
            rm = rm.clone()
        y = native().gn_fwd(_to_form(x.detach(), nhwc), num_groups,
                            weight.detach() if weight is not None else None,
                            bias.detach() if bias is not None else None, float(eps), relu=relu,
                            residual=rm, nhwc=nhwc)[0]
        return _unrows3(y, tuple(x.shape)) if nhwc else y.view(x.shape)
    return _GroupNormFn.apply(x, weight, bias, num_groups, float(eps), relu, residual,
                              residual_grad_into)
