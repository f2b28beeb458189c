"""Differentiable ops over the native gfx950 kernels (CPU tensors use the torch reference)."""
from .activation import gelu, relu6, silu
from .conv import conv2d
from .groupnorm import group_norm
from .excite import se_scale, stochastic_depth
from .layernorm import layer_norm
from .linear import linear
from .loss import backward, count_correct, cross_entropy, linear_cross_entropy, seed_grad
from .norm import batch_norm
from .precision import autocast, is_autocast_enabled
from .pool import adaptive_avg_pool2d, add_relu, dropout, flatten, max_pool2d

__all__ = ["linear", "conv2d", "max_pool2d", "adaptive_avg_pool2d", "dropout", "add_relu",
           "cross_entropy", "linear_cross_entropy", "count_correct", "batch_norm", "backward", "seed_grad", "flatten",
           "autocast", "is_autocast_enabled", "layer_norm", "gelu", "relu6", "silu",
           "se_scale", "stochastic_depth", "group_norm"]
