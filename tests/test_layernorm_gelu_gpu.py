"""LayerNorm and GELU have no gfx950 kernels yet: on a GPU tensor the ops raise, they do not fall
back to ATen."""
import pytest
import torch

import tutorial_torch_distributed_data_parallel_amd as tdp

pytestmark = pytest.mark.gpu


def test_gpu_tensors_raise_instead_of_falling_back():
    x = torch.randn(4, 8, device="cuda")
    with pytest.raises(NotImplementedError, match="layer_norm"):
        tdp.nn.LayerNorm(8, device="cuda")(x)
    with pytest.raises(NotImplementedError, match="gelu"):
        tdp.nn.GELU()(x)
