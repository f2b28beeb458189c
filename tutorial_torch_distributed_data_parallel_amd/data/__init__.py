"""Samplers with the reference's sharding semantics, on-device synthetic data and the host-dataset
pipeline (native prefetcher + on-device resize / flip / normalise)."""
from .augment import (AugmentedTransform, TrivialAugment, affine_params, augment_batch,
                      reference_augment)
from .erase import RandomErasing, erase_boxes, normalize_erase, reference_normalize_erase
from .host import (CIFAR_MEAN, CIFAR_STD, CropTransform, HostImageDataset, ImageTransform,
                   PrefetchLoader, center_crop_boxes, cifar_like_uint8, crop_resize,
                   load_cifar10_bin, pad_crop_boxes, resized_crop_boxes, write_cifar10_bin)
from .mix import BatchMix, mix_batch
from .sampler import BatchShardSampler, DistributedSampler
from .synthetic import DeviceLoader, SyntheticDataset, cifar_like

__all__ = ["DistributedSampler", "BatchShardSampler", "SyntheticDataset", "DeviceLoader",
           "cifar_like", "HostImageDataset", "ImageTransform", "PrefetchLoader",
           "cifar_like_uint8", "load_cifar10_bin", "write_cifar10_bin", "CIFAR_MEAN",
           "CIFAR_STD", "CropTransform", "crop_resize", "resized_crop_boxes", "pad_crop_boxes",
           "center_crop_boxes", "BatchMix", "mix_batch", "augment_batch", "reference_augment",
           "affine_params", "TrivialAugment", "AugmentedTransform", "normalize_erase",
           "reference_normalize_erase", "erase_boxes", "RandomErasing"]
