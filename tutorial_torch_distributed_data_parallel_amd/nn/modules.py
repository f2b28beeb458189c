"""nn.Module front-ends over the native ops (drop-in for the torch modules the reference uses).

Each subclasses its torch counterpart, so parameter names, initialisation, ``state_dict`` keys and
``repr`` are identical to torch's -- checkpoints stay interchangeable with stock PyTorch -- and
only ``forward`` is replaced. ReLU can be fused into the producing layer (``relu=True``), which is
how the models in ``models/`` express torchvision's ``Linear -> ReLU`` pairs.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..parallel import runtime as rt


class Linear(nn.Linear):
    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 relu: bool = False, device=None, dtype=None):
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        self.relu = relu

    def forward(self, x):
        return ops.linear(x, self.weight, self.bias, relu=self.relu)

    def extra_repr(self) -> str:
        return super().extra_repr() + (", relu=True" if self.relu else "")


class Conv2d(nn.Conv2d):
    """``nn.Conv2d`` (dilation=1, zero padding) on the implicit-GEMM kernels, with an optional
    fused ReLU. ``groups > 1`` runs the grouped / depthwise kernels (``ops.conv2d``: channels per
    group multiples of 4, or depthwise with ``in_channels % 4 == 0``)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0,
                 bias: bool = True, relu: bool = False, device=None, dtype=None,
                 groups: int = 1, dilation=1):
        if tuple(nn.modules.utils._pair(dilation)) != (1, 1):
            raise NotImplementedError("Conv2d: dilation is not supported (dilation must be 1)")
        if groups != 1 and device is not None and torch.device(device).type == "cuda":
            # the channel combinations the GPU kernels take: refuse the others here, not at the
            # first forward (a CPU module runs any combination through torch)
            ops.conv.grouped_family(in_channels, out_channels, groups)
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                         groups=groups, bias=bias, device=device, dtype=dtype)
        self.relu = relu
        self.bn_stats = False  # output feeds a BatchNorm: emit its statistics (ops.conv2d)
        # The weight lives in channels_last memory ([Cout][R][S][C]): exactly the operand layout
        # of the implicit-GEMM kernels (forward B, input-gradient taps, weight-gradient output),
        # so no step permutes or copies it. Shape and state_dict keys stay torch's [Cout, C, R, S].
        # (Cg = in_channels / groups: the weight's channel extent.)
        if (in_channels // groups) % 4 == 0:
            self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)

    def forward(self, x, grad_into=None):
        return ops.conv2d(x, self.weight, self.bias, self.stride, self.padding, relu=self.relu,
                          grad_into=grad_into, bn_stats=self.bn_stats and self.training,
                          groups=self.groups)

    def extra_repr(self) -> str:
        # torch's extra_repr shows groups when it is not 1
        return super().extra_repr() + (", relu=True" if self.relu else "")


class ReLU(nn.ReLU):
    """Standalone ReLU (models fuse it into the producer where possible)."""

    def forward(self, x):
        return torch.relu(x)


class ReLU6(nn.ReLU6):
    """Standalone ReLU6 (``ops.relu6``); after a BatchNorm use its ``relu6=True`` instead."""

    def forward(self, x):
        return ops.relu6(x)


class SiLU(nn.SiLU):
    """Standalone SiLU (``ops.silu``: CPU tensors; a GPU tensor raises: no kernel yet)."""

    def forward(self, x):
        return ops.silu(x)


class MaxPool2d(nn.MaxPool2d):
    def forward(self, x):
        return ops.max_pool2d(x, self.kernel_size, self.stride, self.padding)


class AdaptiveAvgPool2d(nn.AdaptiveAvgPool2d):
    def forward(self, x):
        return ops.adaptive_avg_pool2d(x, self.output_size)


class Dropout(nn.Dropout):
    def forward(self, x):
        return ops.dropout(x, self.p, self.training)


class _NativeBN(nn.modules.batchnorm._BatchNorm):
    """Shared forward for BatchNorm{1,2}d / SyncBatchNorm."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True,
                 track_running_stats=True, relu: bool = False, device=None, dtype=None,
                 relu6: bool = False, silu: bool = False):
        if relu and relu6:
            raise ValueError("BatchNorm: relu and relu6 are mutually exclusive")
        if silu and (relu or relu6):
            raise ValueError("BatchNorm: relu, relu6 and silu are mutually exclusive")
        super().__init__(num_features, eps, momentum, affine, track_running_stats,
                         device=device, dtype=dtype)
        self.relu = relu
        self.relu6 = relu6  # fused min(max(y, 0), 6) (MobileNetV2's activation)
        self.silu = silu  # y * sigmoid(y) (EfficientNet's activation; CPU tensors, no residual)
        self._nbt = 0  # host mirror of num_batches_tracked: no device->host sync per step

    def _group(self):
        return None

    def relu_join(self, x, residual, grad_into=None):
        """``relu(bn(x) + residual)`` (ReLU6 on a ``relu6`` module) as one normalisation pass
        (ResNet's residual join);
        ``grad_into``: the residual's gradient goes into that ``SharedGrad``."""
        return self.forward(x, residual, relu=True, residual_grad_into=grad_into)

    def forward(self, x, residual=None, relu=None, residual_grad_into=None):
        """``act?(bn(x) [+ residual])``; ``residual`` fuses a residual join into the
        normalisation (ResNet's ``relu(bn3(conv3(.)) + identity)``, one pass instead of two).
        ``relu`` switches the module's activation (ReLU, ReLU6 on a ``relu6`` module, SiLU on a
        ``silu`` module) on or off for this call."""
        self._check_input_dim(x)
        use_batch = self.training or not self.track_running_stats
        factor = 0.0
        nbt = None
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            if x.is_cuda:
                nbt = self.num_batches_tracked  # incremented by the merge kernel (no ATen add_)
            else:
                self.num_batches_tracked.add_(1)
            self._nbt += 1
            factor = (1.0 / self._nbt) if self.momentum is None else self.momentum
        rm = self.running_mean if (not self.training or self.track_running_stats) else None
        rv = self.running_var if (not self.training or self.track_running_stats) else None
        # `relu` switches the module's own activation off (False) or on (True): on a relu6
        # module "on" is the ReLU6, never a silent plain ReLU
        own6 = getattr(self, "relu6", False)
        own_s = getattr(self, "silu", False)
        on = (self.relu or own6 or own_s) if relu is None else bool(relu)
        return ops.batch_norm(x, rm, rv, self.weight, self.bias, training=use_batch,
                              momentum=factor, eps=self.eps, relu=on and not (own6 or own_s),
                              group=self._group() if use_batch else None, residual=residual,
                              num_batches_tracked=nbt, residual_grad_into=residual_grad_into,
                              relu6=on and own6, silu=on and own_s)

    def extra_repr(self) -> str:
        return super().extra_repr() + (", relu=True" if self.relu else "") + \
            (", relu6=True" if getattr(self, "relu6", False) else "") + \
            (", silu=True" if getattr(self, "silu", False) else "")


class BatchNorm1d(_NativeBN):
    def _check_input_dim(self, x):
        if x.dim() not in (2, 3):
            raise ValueError(f"expected 2D or 3D input (got {x.dim()}D input)")


class BatchNorm2d(_NativeBN):
    def _check_input_dim(self, x):
        if x.dim() != 4:
            raise ValueError(f"expected 4D input (got {x.dim()}D input)")


class SyncBatchNorm(_NativeBN):
    """Batch statistics over the whole job (README pitfall, REF/README.md:79-81).

    Synchronises only in training mode with world_size > 1 (torch semantics,
    TORCH/nn/modules/batchnorm.py:744-839); otherwise it is a plain batch norm.
    """

    def _check_input_dim(self, x):
        if x.dim() < 2:
            raise ValueError(f"expected at least 2D input (got {x.dim()}D input)")

    def _group(self):
        if self.training and rt.is_initialized() and rt.get_world_size() > 1:
            return rt.SyncGroup()
        return None

    @classmethod
    def convert_sync_batchnorm(cls, module: nn.Module, process_group=None) -> nn.Module:
        """Recursively replace every BatchNorm*D (torch's or ours) with SyncBatchNorm."""
        out = module
        if isinstance(module, nn.modules.batchnorm._BatchNorm) and not isinstance(module, cls):
            out = cls(module.num_features, module.eps, module.momentum, module.affine,
                      module.track_running_stats, relu=getattr(module, "relu", False),
                      relu6=getattr(module, "relu6", False),
                      silu=getattr(module, "silu", False))
            if module.affine:
                with torch.no_grad():
                    out.weight = module.weight
                    out.bias = module.bias
            out.running_mean = module.running_mean
            out.running_var = module.running_var
            out.num_batches_tracked = module.num_batches_tracked
            out._nbt = getattr(module, "_nbt", 0)
            out.training = module.training
        for name, child in module.named_children():
            out.add_module(name, cls.convert_sync_batchnorm(child, process_group))
        return out


class GroupNorm(nn.GroupNorm):
    """``nn.GroupNorm`` on the native kernels (``ops.group_norm``), with an optional fused ReLU
    (``relu=True``) and residual join. Per-sample statistics: no collective under data
    parallelism and nothing for ``convert_sync_batchnorm`` to convert; training and eval are the
    same computation. ``state_dict`` keys, init and ``extra_repr`` are torch's."""

    def __init__(self, num_groups: int, num_channels: int, eps: float = 1e-5,
                 affine: bool = True, relu: bool = False, device=None, dtype=None):
        super().__init__(num_groups, num_channels, eps=eps, affine=affine, device=device,
                         dtype=dtype)
        self.relu = relu

    def relu_join(self, x, residual, grad_into=None):
        """``relu(gn(x) + residual)`` as one normalisation pass (ResNet's residual join);
        ``grad_into``: the residual's gradient goes into that ``SharedGrad``."""
        return self.forward(x, residual, relu=True, residual_grad_into=grad_into)

    def forward(self, x, residual=None, relu=None, residual_grad_into=None):
        """``relu?(gn(x) [+ residual])``; ``relu`` overrides the module's own setting for this
        call."""
        on = self.relu if relu is None else bool(relu)
        return ops.group_norm(x, self.num_groups, self.weight, self.bias, self.eps, relu=on,
                              residual=residual, residual_grad_into=residual_grad_into)

    def extra_repr(self) -> str:
        return super().extra_repr() + (", relu=True" if self.relu else "")


class LayerNorm(nn.LayerNorm):
    """``nn.LayerNorm`` through ``ops.layer_norm`` (CPU tensors; a GPU tensor raises: no kernel
    yet)."""

    def forward(self, x):
        return ops.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)


class GELU(nn.GELU):
    def forward(self, x):
        return ops.gelu(x, approximate=self.approximate)


class StochasticDepth(nn.Module):
    """torchvision's ``StochasticDepth(p, mode)`` (``ops.stochastic_depth``); ``"row"`` only."""

    def __init__(self, p: float, mode: str = "row"):
        super().__init__()
        if mode != "row":
            raise NotImplementedError(f"StochasticDepth: only mode='row' is supported, got "
                                      f"{mode!r}")
        self.p = p
        self.mode = mode

    def forward(self, x):
        return ops.stochastic_depth(x, self.p, self.training)

    def extra_repr(self) -> str:
        return f"p={self.p}, mode={self.mode}"


class SqueezeExcitation(nn.Module):
    """torchvision's ``SqueezeExcitation(input_channels, squeeze_channels)`` with SiLU inside and
    a sigmoid gate: global average pool (the NHWC kernel), ``fc1`` and ``fc2`` as 1x1 ``Conv2d``
    with bias on the [N, C, 1, 1] map (keys ``fc1.weight [sq, C, 1, 1]``, ``fc1.bias``,
    ``fc2.*``), the stand-alone SiLU between them, and ``ops.se_scale`` for the gate. CPU
    tensors only so far: ``ops.silu`` and ``ops.se_scale`` have no gfx950 kernels yet and raise
    on a GPU tensor. Fusing the squeeze into the producing BatchNorm pass is a follow-up."""

    def __init__(self, input_channels: int, squeeze_channels: int, device=None):
        super().__init__()
        self.fc1 = Conv2d(input_channels, squeeze_channels, 1, device=device)
        self.fc2 = Conv2d(squeeze_channels, input_channels, 1, device=device)

    def forward(self, x):
        t = ops.adaptive_avg_pool2d(x, 1)
        t = self.fc2(ops.silu(self.fc1(t)))
        return ops.se_scale(x, t)


class CrossEntropyLoss(nn.CrossEntropyLoss):
    def forward(self, input, target):
        if self.weight is not None:
            raise NotImplementedError("class weights are not supported by the native loss")
        return ops.cross_entropy(input, target, ignore_index=self.ignore_index,
                                 label_smoothing=self.label_smoothing, reduction=self.reduction)


convert_sync_batchnorm = SyncBatchNorm.convert_sync_batchnorm
