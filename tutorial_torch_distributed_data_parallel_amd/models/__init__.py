"""Model zoo: the flagship toy MLP (+SyncBN variant), AlexNet (reference), ResNet-50, ResNeXt-50,
MLP-Mixer, MobileNetV2 and EfficientNet-B0 (``registry.build_model`` builds them by name)."""
from .efficientnet import EfficientNet, efficientnet_b0
from .mlp import ToyMLP, toy_mlp

__all__ = ["ToyMLP", "toy_mlp", "EfficientNet", "efficientnet_b0"]
