"""bf16 mixed precision: a thread-local autocast flag the Linear and convolution ops read at
forward time.

The contract is the standard one: bf16 operands, fp32 accumulation, fp32 master weights and
optimizer state. Under ``autocast`` a float32 Linear (``ops/linear.py``) or convolution
(``ops/conv.py``) rounds each operand element once to bf16 (round-to-nearest-even) and runs its
forward, input-gradient and weight-gradient GEMMs as single bf16 MFMA products with fp32
accumulation (``csrc/gemm_bf16.hip``; ``csrc/conv_bf16.hip``, the same tile with implicit
operand loaders); tensors stay float32 in memory, the bias gradient is summed from the unrounded
output gradient, and the loss is float32.

What stays fp32 under autocast: BatchNorm (which then runs its own moments pass: the bf16
convolution has no statistics epilogue yet), pooling, dropout, the losses, the optimizers, and
the convolutions the channels_last path does not take (channel counts that are not a multiple
of 4 beyond the stem, non-power-of-two strides with an input gradient): those run the fp32 NCHW
fallback, bitwise equal to the result outside autocast. Grouped and depthwise convolutions
(``groups > 1``, csrc/conv_grouped.hip) have no bf16 form and stay fp32 too, bitwise equal to the
result outside autocast. ``ops.conv.AUTOCAST_FP32_CONV = True``
keeps every convolution fp32 (A/B measurement).

The op is chosen in forward, so a layer's backward follows its forward whether or not the flag
is still on when ``loss.backward()`` runs.
"""
from __future__ import annotations

import functools
import threading

import torch

_state = threading.local()


def is_autocast_enabled() -> bool:
    """The calling thread is inside an enabled :class:`autocast` region."""
    return getattr(_state, "on", False)


class autocast:
    """Context manager / decorator: Linear and convolution layers compute in bf16 mixed
    precision (fp32 tensors, operands rounded once per GEMM pass, fp32 accumulation).

    Re-entrant and nestable (``autocast(enabled=False)`` inside an enabled region turns it off
    for that block); the previous state is restored on exit, exceptions included. Only
    ``torch.bfloat16`` is supported.
    """

    def __init__(self, enabled: bool = True, dtype: torch.dtype = torch.bfloat16):
        if dtype != torch.bfloat16:
            raise ValueError(f"autocast supports dtype=torch.bfloat16 only, got {dtype}")
        self.enabled = bool(enabled)
        self.dtype = dtype
        self._prev = []

    def __enter__(self):
        self._prev.append(is_autocast_enabled())
        _state.on = self.enabled
        return self

    def __exit__(self, *exc):
        _state.on = self._prev.pop()
        return False

    def __call__(self, fn):
        @functools.wraps(fn)
        def wrapped(*a, **k):
            with autocast(self.enabled, self.dtype):
                return fn(*a, **k)

        return wrapped
