"""MLP-Mixer (Tolstikhin et al., 2021): the smallest model family that needs LayerNorm and GELU
and nothing else -- Linear, LayerNorm, GELU and residual adds, no attention.

    stem   : Conv2d(3, dim, patch, stride=patch)        [B, 3, S, S] -> [B, T, dim], T = (S/patch)^2
    block  : x = x + tokens_mlp(LN(x)^T)^T              (mixes the T tokens, per channel)
             x = x + channels_mlp(LN(x))                (mixes the dim channels, per token)
    head   : LN, mean over tokens, Linear(dim, num_classes)

Each MLP is Linear - GELU - Linear. The convolution's output is channels_last on the GPU, so
``[B, dim, H, W] -> [B, T, dim]`` is a view of the same memory (no copy). The two token-mixing
transposes are torch copies (a transposing LayerNorm store would remove the first).

The model runs on CPU tensors (plain and under gloo DDP). LayerNorm and GELU have no gfx950
kernels yet, so a forward on the GPU raises at the first LayerNorm.
"""
from __future__ import annotations

import torch.nn as nn

from ..nn import GELU, Conv2d, LayerNorm, Linear


class MixerMlp(nn.Module):
    def __init__(self, features: int, hidden: int, device=None):
        super().__init__()
        self.fc1 = Linear(features, hidden, device=device)
        self.act = GELU()
        self.fc2 = Linear(hidden, features, device=device)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class MixerBlock(nn.Module):
    def __init__(self, tokens: int, dim: int, tokens_mlp: int, channels_mlp: int, device=None):
        super().__init__()
        self.norm1 = LayerNorm(dim, device=device)
        self.token_mlp = MixerMlp(tokens, tokens_mlp, device=device)
        self.norm2 = LayerNorm(dim, device=device)
        self.channel_mlp = MixerMlp(dim, channels_mlp, device=device)

    def forward(self, x):  # [B, T, dim]
        x = x + self.token_mlp(self.norm1(x).transpose(1, 2)).transpose(1, 2)
        return x + self.channel_mlp(self.norm2(x))


class MlpMixer(nn.Module):
    def __init__(self, image_size: int = 224, patch: int = 16, dim: int = 512, depth: int = 8,
                 tokens_mlp: int = 256, channels_mlp: int = 2048, num_classes: int = 10,
                 device=None):
        super().__init__()
        if image_size % patch:
            raise ValueError(f"image_size {image_size} is not a multiple of patch {patch}")
        self.image_size = image_size
        tokens = (image_size // patch) ** 2
        self.stem = Conv2d(3, dim, patch, stride=patch, device=device)
        self.blocks = nn.Sequential(*[MixerBlock(tokens, dim, tokens_mlp, channels_mlp, device)
                                      for _ in range(depth)])
        self.norm = LayerNorm(dim, device=device)
        self.head = Linear(dim, num_classes, device=device)

    def forward(self, x):
        x = self.stem(x)  # [B, dim, H, W], channels_last on the GPU
        B, dim = x.shape[0], x.shape[1]
        x = x.permute(0, 2, 3, 1).reshape(B, -1, dim)  # a view of channels_last memory
        x = self.blocks(x)
        return self.head(self.norm(x).mean(dim=1))


def mixer_s16(num_classes: int = 10, device=None, image_size: int = 224) -> MlpMixer:
    return MlpMixer(image_size, 16, 512, 8, 256, 2048, num_classes, device)


def mixer_b16(num_classes: int = 10, device=None, image_size: int = 224) -> MlpMixer:
    return MlpMixer(image_size, 16, 768, 12, 384, 3072, num_classes, device)
