"""2-D convolution (+ fused bias / ReLU) on the native implicit-GEMM MFMA kernels.

Replaces MIOpen for the CNN models (§2.5 K1/K4/K6-K8 forward, K22 backward;
torchvision AlexNet features, REF/data_and_toy_model.py:41-45; ResNet-50 for the "ResNet-50-sized
CNN" config). No im2col buffer is ever materialised.

Main path -- channels_last (NHWC) activations on the LDS-DMA MFMA GEMM pipeline
(``csrc/gemm_f32_fast.hip``, implicit operand sources):
  * forward  ``y[(n,p,q)][co] = relu?(sum_(r,s,c) x[n][p*sh-ph+r][q*sw-pw+s][c] * W[co][c][r][s] + b)``
    -- K is ordered (r, s, c) so every 16-B DMA chunk is 4 contiguous channels of one pixel;
  * input gradient -- the same gather on ``dy`` with the transpose-stride test;
  * weight gradient -- ``dy^T`` (a plain [pixels][Cout] matrix) times shifted-pixel rows of ``x``,
    split-K over the N*P*Q reduction.
  Outputs are channels_last, so a 1x1 convolution IS a GEMM ([N*H*W, C] x [C, Cout]); batch norm
  and the ReLU/bias backward treat NHWC tensors as [pixels, C] matrices. Weights are
  channels_last parameters (logical [Cout, C, R, S]: state_dict / checkpoints unchanged) whose
  [Cout][R][S][C] memory every kernel reads or writes directly (see _ConvNHWCFn).
  Input channels that are not a multiple of 4 (the RGB stem) are zero-padded to 4, natively.
Fallback -- NCHW register-staged implicit GEMM (``csrc/conv.hip``) for shapes the NHWC path does
not take (channel counts not a multiple of 4 beyond the stem, non power-of-two strides in dgrad).
CPU tensors run ``torch.nn.functional.conv2d`` (the oracle of the CPU tests).
Dilation is not supported (no model here uses it).

Groups -- ``groups > 1`` runs ``csrc/conv_grouped.hip`` (``_ConvGroupedFn``): NHWC, fp32 FMA on the
VALU, the same channels_last weight memory in all three passes, the weight gradient written
straight into the parameter's gradient slot. Two families: grouped (Cin/groups and Cout/groups
multiples of 4; ResNeXt, two-tower AlexNet) and depthwise (groups == Cin, Cout = m * Cin,
Cin % 4 == 0; a register-tap stencil). Any other channel combination raises
``NotImplementedError``. No bf16 form: inside ``tdp.autocast`` a grouped convolution stays fp32,
bitwise equal to the result outside it. ``bn_stats`` produces nothing for the grouped family and
for the generic depthwise form; the register-tap depthwise forward (3x3 / 5x5, channel multiplier
1, no bias, no fused ReLU) has a statistics epilogue behind ``DW_BN_STATS``: each block reduces
its own pixels per channel in LDS in a fixed order and writes one (count, mean, M2) partial per
(block, channel), the ``[T, 3, C]`` layout ``bn_moments_partials`` consumes, so BatchNorm skips its
moments pass over the output. The output is bitwise the one without the epilogue.
``groups == 1`` never reaches this code.

Mixed precision -- inside ``tdp.autocast`` (ops/precision.py) a float32 convolution the NHWC
path takes runs its three passes on ``csrc/conv_bf16.hip``: the same implicit GEMMs with every
operand element rounded once to bf16 (round-to-nearest-even), exact products, fp32 accumulation
and fp32 tensors in memory. The ReLU mask and the bias gradient come from the unrounded output
gradient (``relu_bias_bwd``); its result is what the two gradient GEMMs round. The op family is
chosen in forward and the backward follows it. The stem padding, the weight-gradient
destination, the stride phases and the shared-gradient sink are the fp32 path's own code
(``_ConvNHWCFn`` with ``bf16=True``). Under autocast the GEMM epilogue does not produce the
BatchNorm statistics (``bn_stats``): BatchNorm runs its own moments pass; a statistics epilogue
for the bf16 kernel is a follow-up. Shapes the NHWC path does not take (see Fallback) stay
fp32 under autocast, bitwise equal to the result outside it. CPU tensors under autocast run the
same contract in torch math (``_ConvBf16CpuFn``). ``AUTOCAST_FP32_CONV = True`` keeps every
convolution fp32 under autocast (A/B measurement).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .._native import native
from . import plan_db
from ._grad import SharedGrad, grad_dest, needs
from .precision import is_autocast_enabled


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, relu: bool, sink=None):
        C = native()
        sh, sw = stride
        ph, pw = padding
        y = C.conv2d_fwd(x, weight, bias, sh, sw, ph, pw, relu)
        ctx.sink = sink
        ctx.geom = (sh, sw, ph, pw)
        ctx.relu = relu
        ctx.params = (weight, bias)
        ctx.x_shape = list(x.shape)
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = native()
        x, weight, y = ctx.saved_tensors
        w_param, b_param = ctx.params
        sh, sw, ph, pw = ctx.geom
        dy = dy.contiguous()
        want_db = b_param is not None and needs(ctx, 2)
        db = grad_dest(b_param) if want_db else None
        # one pass: ReLU mask (g = dy * (y > 0)) and the per-channel bias gradient
        if ctx.relu or want_db:
            g = C.chan_relu_bias_bwd(dy, y if ctx.relu else None, db)
        else:
            g = dy
        dx = dw = None
        if needs(ctx, 1):
            dw = grad_dest(w_param)
            C.conv2d_wgrad(g, x, dw, sh, sw, ph, pw, 0.0)
        if needs(ctx, 0):
            dx = C.conv2d_dgrad(g, weight, ctx.x_shape, sh, sw, ph, pw)
            if ctx.sink is not None:
                dx = ctx.sink.deposit(dx)
        return dx, dw, db, None, None, None, None


_CL = torch.channels_last


def _rows(t):
    """[N, C, H, W] channels_last tensor -> its [N*H*W, C] storage as a 2-D view."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _as_cl(C, t, channels: int | None = None):
    """``t`` as a channels_last tensor with ``channels`` channels (zero-padded): ``t`` itself
    when it already is one, else ONE native strided copy (csrc/elementwise.hip copy4d)."""
    n, c, h, w = t.shape
    channels = c if channels is None else channels
    if channels == c and t.is_contiguous(memory_format=_CL):
        return t
    base = getattr(t, "_tdp_padded_base", None)
    if base is not None and tuple(base.shape) == (n, h, w, channels) and \
            t.data_ptr() == base.data_ptr() and t.stride() == (h * w * channels, 1, w * channels,
                                                                 channels):
        # a channel-padded channels_last batch (data/synthetic.py): its zero-filled storage IS
        # the padded NHWC operand
        return base.permute(0, 3, 1, 2)
    out = torch.empty((n, channels, h, w), device=t.device, dtype=t.dtype, memory_format=_CL)
    C.copy4d(out, t)
    return out


class _ConvNHWCFn(torch.autograd.Function):
    """Weights are channels_last parameters ([Cout][R][S][C] memory, nn/modules.py Conv2d): the
    forward reads them as the GEMM's K-contiguous B, the input gradient gathers its taps straight
    from them (csrc/gemm_f32_fast.hip WTap), and the weight gradient is written straight into
    the parameter's gradient slot in that layout -- no per-step permute / pad / copy-back. Only
    the RGB stem (3 channels, padded to 4 for the 16-B DMA chunks) repacks, natively."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, relu: bool, sink=None, stats_box=None,
                bf16: bool = False):
        # bf16: every GEMM of the three passes on the mixed-precision kernels (csrc/conv_bf16.hip)
        C = native()
        N, Cin, H, W = x.shape
        Cout, _, R, S = weight.shape
        Cp = (Cin + 3) // 4 * 4
        sh, sw = stride
        ph, pw = padding
        xp = _as_cl(C, x, Cp)
        wt = _as_cl(C, weight, Cp)  # the parameter itself for every conv but the stem
        if bf16:
            if stats_box is not None:
                stats_box.append(None)  # no statistics epilogue: BatchNorm takes its own moments
            y = C.conv_nhwc_fwd(xp, wt.permute(0, 2, 3, 1), bias, R, S, sh, sw, ph, pw, relu,
                                bf16=True)
        elif stats_box is not None and bias is None and not relu:
            # the GEMM epilogue also emits the output's per-tile BN statistics (or None)
            y, st = C.conv_nhwc_fwd_stats(xp, wt.permute(0, 2, 3, 1), R, S, sh, sw, ph, pw)
            stats_box.append(st)
        else:
            y = C.conv_nhwc_fwd(xp, wt.permute(0, 2, 3, 1), bias, R, S, sh, sw, ph, pw, relu)
        ctx.geom = (R, S, sh, sw, ph, pw, Cin, Cp)
        ctx.sink = sink
        ctx.relu = relu
        ctx.bf16 = bf16
        ctx.params = (weight, bias)
        ctx.save_for_backward(xp, wt, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = native()
        xp, wt, y = ctx.saved_tensors
        w_param, b_param = ctx.params
        R, S, sh, sw, ph, pw, Cin, Cp = ctx.geom
        Cout = wt.shape[0]
        bf16 = ctx.bf16
        dy = _as_cl(C, dy)
        want_db = b_param is not None and needs(ctx, 2)
        db = grad_dest(b_param) if want_db else None
        # ReLU mask + bias gradient: one pass over dy viewed as [pixels, Cout]
        if ctx.relu or want_db:
            g2 = C.relu_bias_bwd(_rows(dy), _rows(y) if ctx.relu else None, db)
            g = g2.view(dy.shape[0], dy.shape[2], dy.shape[3], Cout).permute(0, 3, 1, 2)
        else:
            g = dy
        dx = dw = None
        if needs(ctx, 1):
            dw = grad_dest(w_param)
            if not bf16 and C.conv_wgrad_transposed(Cout, R, S, Cp):
                # dW^T [(r,s,c)][co] when it pads the 128-row MFMA tiles less (small Cout, Cout=192)
                dwT = torch.empty((R, S, Cp, Cout), device=dy.device, dtype=dy.dtype)
                C.conv_nhwc_wgrad(g, xp, dwT, R, S, sh, sw, ph, pw, 0.0)
                C.copy4d(dw, dwT.permute(3, 2, 0, 1))
            elif Cp == Cin and dw.permute(0, 2, 3, 1).is_contiguous():
                # straight into the gradient slot ([Cout][R][S][C] = the parameter's layout)
                C.conv_nhwc_wgrad(g, xp, dw.permute(0, 2, 3, 1), R, S, sh, sw, ph, pw, 0.0,
                                  bf16=bf16)
            else:
                dwt = torch.empty((Cout, R, S, Cp), device=dy.device, dtype=dy.dtype)
                C.conv_nhwc_wgrad(g, xp, dwt, R, S, sh, sw, ph, pw, 0.0, bf16=bf16)
                C.copy4d(dw, dwt.permute(0, 3, 1, 2))
        if needs(ctx, 0):
            sink = ctx.sink
            acc = sink.buf if (sink is not None and Cp == Cin) else None
            if sh == 1 and sw == 1:
                # with a shared residual-input gradient: accumulated by the GEMM (beta = 1)
                dx = C.conv_nhwc_dgrad_w(g, wt, list(xp.shape), sh, sw, ph, pw, out=acc,
                                         beta=0.0 if acc is None else 1.0, bf16=bf16)
            else:
                dx = _dgrad_phases(C, g, wt, xp.shape, R, S, sh, sw, ph, pw, into=acc, bf16=bf16)
            if Cp != Cin:
                dx = dx[:, :Cin]
            if sink is not None:
                dx = dx if acc is not None else sink.deposit(dx)
        return dx, dw, db, None, None, None, None, None, None


def _dgrad_phases(C, g, wt, x_shape, R, S, sh, sw, ph, pw, into=None, bf16=False):
    """Strided input gradient as sh*sw stride-1 GEMMs, one per output phase.

    dx pixels h = a + sh*i only receive taps r = r0 + sh*t with r0 = (a + ph) mod sh, from dy row
    p = i + da - t (da = (a + ph - r0) / sh): a stride-1 convolution over the phase sub-grid with
    the phase's taps, which the kernel gathers from the weight itself. This skips the
    (sh*sw - 1)/(sh*sw) of multiply-adds a direct gather spends on the zeros between strided
    taps (measured 4x on ResNet's stride-2 layers). ``into``: accumulate into that tensor
    instead (phases without taps leave it alone)."""
    N, Cp, H, W = x_shape
    acc = into is not None
    dx = into if acc else torch.empty(x_shape, device=g.device, dtype=g.dtype, memory_format=_CL)
    none = torch.empty((0, 0, 0, 0), device=g.device, dtype=g.dtype)
    for a in range(sh):
        r0 = (a + ph) % sh
        Rp, Hp, da = len(range(r0, R, sh)), len(range(a, H, sh)), (a + ph - r0) // sh
        for b in range(sw):
            s0 = (b + pw) % sw
            Sp, Wp, db = len(range(s0, S, sw)), len(range(b, W, sw)), (b + pw - s0) // sw
            if Hp == 0 or Wp == 0:
                continue
            view = dx[:, :, a::sh, b::sw]
            if Rp == 0 or Sp == 0:
                if not acc:
                    C.copy4d(view, none)  # no tap reaches this phase: zeros
                continue
            C.copy4d(view, C.conv_nhwc_dgrad_phase_w(g, wt, Hp, Wp, Rp, Sp, da, db, r0, s0, sh,
                                                     sw, bf16=bf16), accumulate=acc)
    return dx


FORCE_NCHW = False  # tests: route every conv through the NCHW fallback kernels
AUTOCAST_FP32_CONV = False  # A/B measurement: convolutions stay fp32 inside tdp.autocast
# bn_stats on a register-tap depthwise forward emits the BatchNorm statistics from the kernel
# (False: BatchNorm runs its moments pass, A/B measurement). On: over MobileNetV2's depthwise
# layers forward + epilogue + merge takes 475 us against 515 us for forward + moments pass, and
# the eager step is not slower (profiles/r18/mobilenet_v2.md).
DW_BN_STATS = True


def _bf16r(t: torch.Tensor) -> torch.Tensor:
    """``t`` with every element rounded to bf16 (round-to-nearest-even), as float32."""
    return t.bfloat16().float()


class _ConvBf16CpuFn(torch.autograd.Function):
    """The bf16 contract of the device path in torch math (CPU tensors under autocast): each
    pass rounds its operands once, the ReLU mask and the bias gradient use the unrounded g."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, relu: bool):
        y = F.conv2d(_bf16r(x), _bf16r(weight), bias, stride, padding)
        if relu:
            y = F.relu(y)
        ctx.geom = (stride, padding)
        ctx.relu = relu
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        stride, padding = ctx.geom
        g = dy * (y > 0) if ctx.relu else dy
        gr = _bf16r(g)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.nn.grad.conv2d_input(x.shape, _bf16r(weight), gr, stride, padding)
        if ctx.needs_input_grad[1]:
            dw = torch.nn.grad.conv2d_weight(_bf16r(x), weight.shape, gr, stride, padding)
        if ctx.needs_input_grad[2]:
            db = g.sum(dim=(0, 2, 3))
        return dx, dw, db, None, None, None


GROUPS_RULE = (
    "native grouped convolution takes (a) grouped: groups > 1 with Cin/groups and Cout/groups "
    "both multiples of 4, or (b) depthwise: groups == Cin (Cout = m * Cin, channel multiplier "
    "m >= 1) with Cin a multiple of 4")


def grouped_family(cin: int, cout: int, groups: int) -> str:
    """``"grouped"`` or ``"depthwise"``: the kernel family of csrc/conv_grouped.hip that takes
    ``(cin, cout, groups)``; any other combination raises ``NotImplementedError`` (there is no
    slow path)."""
    if groups < 1 or cin % groups or cout % groups:
        raise ValueError(f"conv2d: Cin={cin} and Cout={cout} must be divisible by groups={groups}")
    cg, kg = cin // groups, cout // groups
    if groups > 1 and cg == 1 and cin % 4 == 0:
        return "depthwise"
    if groups > 1 and cg > 1 and cg % 4 == 0 and kg % 4 == 0:
        return "grouped"
    raise NotImplementedError(f"conv2d(Cin={cin}, Cout={cout}, groups={groups}): {GROUPS_RULE}")


class _ConvGroupedFn(torch.autograd.Function):
    """Grouped / depthwise convolution on csrc/conv_grouped.hip (fp32 FMA, NHWC). As in
    ``_ConvNHWCFn`` the weight operand of all three passes is the parameter's own channels_last
    memory ([Cout][R][S][Cg]) and the weight gradient is written straight into the parameter's
    gradient slot; the ReLU mask and the bias gradient are the shared ``relu_bias_bwd`` pass."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, groups: int, relu: bool, sink=None,
                stats_box=None):
        C = native()
        xc = _as_cl(C, x)
        wt = _as_cl(C, weight)  # the parameter itself when it is stored channels_last
        if stats_box is not None:
            # depthwise, no bias, no ReLU: the stencil also emits the per-block BN statistics
            # (None when the geometry has no statistics form)
            r = C.conv_dw_fwd_stats(xc, wt, *stride, *padding, groups)
            y = r[0]
            stats_box.append(r[1] if len(r) > 1 else None)
        else:
            y = C.conv_grouped_fwd(xc, wt, bias, *stride, *padding, groups, relu)
        ctx.geom = (*stride, *padding, groups)
        ctx.sink = sink
        ctx.relu = relu
        ctx.params = (weight, bias)
        ctx.save_for_backward(xc, wt, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        C = native()
        xc, wt, y = ctx.saved_tensors
        w_param, b_param = ctx.params
        geom = ctx.geom
        Cout = wt.shape[0]
        dy = _as_cl(C, dy)
        want_db = b_param is not None and needs(ctx, 2)
        db = grad_dest(b_param) if want_db else None
        if ctx.relu or want_db:
            g2 = C.relu_bias_bwd(_rows(dy), _rows(y) if ctx.relu else None, db)
            g = g2.view(dy.shape[0], dy.shape[2], dy.shape[3], Cout).permute(0, 3, 1, 2)
        else:
            g = dy
        dx = dw = None
        if needs(ctx, 1):
            dw = grad_dest(w_param)
            if dw.permute(0, 2, 3, 1).is_contiguous():
                C.conv_grouped_wgrad(g, xc, dw, *geom)  # straight into the gradient slot
            else:
                dwt = torch.empty_like(wt)
                C.conv_grouped_wgrad(g, xc, dwt, *geom)
                C.copy4d(dw, dwt)
        if needs(ctx, 0):
            sink = ctx.sink
            acc = sink.buf if sink is not None else None
            if acc is not None and not acc.is_contiguous(memory_format=_CL):
                acc = None
            # with a shared residual-input gradient: accumulated by the kernel's epilogue
            dx = C.conv_grouped_dgrad(g, wt, list(xc.shape), *geom, out=acc,
                                      accumulate=acc is not None)
            if sink is not None and acc is None:
                dx = sink.deposit(dx)
        return dx, dw, db, None, None, None, None, None, None


def _nhwc_ok(x, weight, stride):
    if FORCE_NCHW:
        return False
    Cin, Cout = weight.shape[1], weight.shape[0]
    pow2 = all(s > 0 and (s & (s - 1)) == 0 for s in stride)
    return (Cin % 4 == 0 or Cin < 4) and Cout % 4 == 0 and (pow2 or not x.requires_grad)


def conv2d(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None,
           stride=1, padding=0, relu: bool = False,
           grad_into: SharedGrad | None = None, bn_stats: bool = False,
           groups: int = 1, dilation=1) -> torch.Tensor:
    """``relu?(conv2d(x, weight, bias, stride, padding))`` for float32 [N, C, H, W] tensors.

    On the GPU the result is channels_last (NHWC memory, logical NCHW shape, as torch does for
    channels_last inputs). ``grad_into``: the input gradient goes into that shared buffer (a
    forked residual input, ops/_grad.py ``fork``). ``bn_stats``: the output will be
    batch-normalised -- the GEMM epilogue also computes its per-channel statistics, attached
    to the result for ``batch_norm`` (no moments pass over the output).

    Inside ``tdp.autocast`` a float32 convolution computes in bf16 mixed precision (operands
    rounded once per pass, fp32 accumulation, fp32 tensors; see the module docstring). There
    ``bn_stats`` produces nothing -- BatchNorm runs its own moments pass; a statistics epilogue
    for the bf16 kernel is a follow-up -- and shapes the NHWC path does not take stay fp32.

    ``groups > 1``: grouped or depthwise convolution on csrc/conv_grouped.hip (``weight`` is
    torch's ``[Cout, Cin/groups, R, S]``); ``grouped_family`` states which channel counts are
    taken, any other raises ``NotImplementedError``. ``bn_stats`` produces nothing there -- except,
    with ``DW_BN_STATS``, for a 3x3 / 5x5 depthwise convolution with channel multiplier 1, no bias
    and no ReLU -- and the convolution stays fp32 inside ``tdp.autocast``. ``dilation`` other than 1 is not supported.

    Squeeze-and-excitation (``nn.SqueezeExcitation``) runs its two 1x1 convolutions WITH bias on
    [N, C, 1, 1] maps through this function: N-row problems. EfficientNet-B0's squeeze widths 8, 4,
    20, 28 and 48 take the NHWC path, 6 and 10 (no multiples of 4) the NCHW fallback kernels.
    The module as a whole runs on CPU tensors only so far (its SiLU and gate have no kernels).
    The 4-row NHWC backward with bias (32 -> 8 -> 32) is the suspected, unproven site of the
    fault recorded in profiles/r19/efficientnet_b0.md: read it before relying on that shape."""
    stride, padding = _pair(stride), _pair(padding)
    if _pair(dilation) != (1, 1):
        raise NotImplementedError("conv2d: dilation is not supported (dilation must be 1)")
    if groups != 1:
        if not x.is_cuda:
            y = F.conv2d(x, weight, bias, stride, padding, 1, groups)
            return F.relu(y) if relu else y
        if x.dtype != torch.float32:
            raise TypeError(f"native conv2d expects float32 activations, got {x.dtype}")
        family = grouped_family(x.shape[1], weight.shape[0], groups)
        box = [] if (bn_stats and DW_BN_STATS and family == "depthwise" and bias is None
                     and not relu) else None
        y = _ConvGroupedFn.apply(x, weight, bias, stride, padding, groups, relu, grad_into, box)
        if box and box[0] is not None:
            y._tdp_bn_part = (box[0], y._version)  # ops/norm.py batch_norm consumes it
        return y
    amp = is_autocast_enabled() and x.dtype == torch.float32 and not AUTOCAST_FP32_CONV
    if not x.is_cuda:
        if amp:
            return _ConvBf16CpuFn.apply(x, weight, bias, stride, padding, relu)
        y = F.conv2d(x, weight, bias, stride, padding)
        return F.relu(y) if relu else y
    if x.dtype != torch.float32:
        raise TypeError(f"native conv2d expects float32 activations, got {x.dtype}")
    if _nhwc_ok(x, weight, stride):
        plan_db.ensure_loaded(native())  # measured per-geometry plans (ops/plan_db.py)
        box = [] if bn_stats else None
        y = _ConvNHWCFn.apply(x, weight, bias, stride, padding, relu, grad_into, box, amp)
        if box and box[0] is not None:
            y._tdp_bn_part = (box[0], y._version)  # ops/norm.py batch_norm consumes it
        return y
    return _Conv2dFn.apply(x.contiguous(), weight.contiguous(), bias, stride, padding, relu,
                           grad_into)


def bias_relu_backward_reference(dy, y, bias_needed: bool):
    """CPU oracle of ``chan_relu_bias_bwd`` (used by tests)."""
    g = dy * (y > 0) if y is not None else dy
    db = g.sum(dim=(0, 2, 3)) if bias_needed else None
    return g, db
