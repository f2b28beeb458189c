"""MLP-Mixer in plain torch.nn, module for module the published architecture: the twin the
LayerNorm / GELU / Mixer tests compare ``models/mixer.py`` against (same attribute names, so a
``state_dict`` of either loads into the other)."""
import torch.nn as nn


class TwinMlp(nn.Module):
    def __init__(self, features, hidden):
        super().__init__()
        self.fc1 = nn.Linear(features, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class TwinBlock(nn.Module):
    def __init__(self, tokens, dim, tokens_mlp, channels_mlp):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.token_mlp = TwinMlp(tokens, tokens_mlp)
        self.norm2 = nn.LayerNorm(dim)
        self.channel_mlp = TwinMlp(dim, channels_mlp)

    def forward(self, x):
        x = x + self.token_mlp(self.norm1(x).transpose(1, 2)).transpose(1, 2)
        return x + self.channel_mlp(self.norm2(x))


class TwinMixer(nn.Module):
    def __init__(self, image_size=224, patch=16, dim=512, depth=8, tokens_mlp=256,
                 channels_mlp=2048, num_classes=10):
        super().__init__()
        tokens = (image_size // patch) ** 2
        self.stem = nn.Conv2d(3, dim, patch, stride=patch)
        self.blocks = nn.Sequential(*[TwinBlock(tokens, dim, tokens_mlp, channels_mlp)
                                      for _ in range(depth)])
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(dim, num_classes)

    def forward(self, x):
        x = self.stem(x).flatten(2).transpose(1, 2)  # [B, T, dim]
        x = self.blocks(x)
        return self.head(self.norm(x).mean(dim=1))


SMALL = dict(image_size=32, patch=8, dim=64, depth=2, tokens_mlp=32, channels_mlp=128)
S16 = dict(image_size=224, patch=16, dim=512, depth=8, tokens_mlp=256, channels_mlp=2048)
B16 = dict(image_size=224, patch=16, dim=768, depth=12, tokens_mlp=384, channels_mlp=3072)
