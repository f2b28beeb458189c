"""Host-dataset input pipeline (the reference's CIFAR-10 + torchvision transforms + DataLoader).

Reference (REF/data_and_toy_model.py:8-38, REF/multi-GPU-training-torch.py:86-99): CIFAR-10 as
PIL uint8 32x32 images, ``Resize(224) -> RandomHorizontalFlip -> ToTensor -> Normalize(mean,
std)`` per sample in 2 DataLoader worker processes per rank, ``pin_memory=True``, then a 77 MB
float32 H2D copy per 128-sample batch.

Here:
  * ``HostImageDataset`` keeps the samples as ONE uint8 ``[n, H, W, C]`` host tensor (or a
    ``numpy.memmap`` of one) -- 150 MB for the whole CIFAR-10 training set;
  * ``PrefetchLoader`` hands the sampler's epoch order to the native ``HostBatchLoader``
    (csrc/loader.h): C++ worker threads gather the sampled rows into pinned staging slots
    ``depth`` batches ahead, with per-sample flip bits from a counter-based hash of
    (seed, epoch, position);
  * per step one async H2D copy of the uint8 batch (393 KB at 32x32, 200x less than the
    reference's float batch) on the current stream, then ``image_transform`` (csrc/image.hip)
    does resize + flip + /255 + normalise in one pass on the GPU and writes the channels_last
    float batch the convolutions consume.
  * ``CropTransform`` is the training-recipe variant: per-sample boxes (RandomResizedCrop,
    RandomCrop(padding) or a centre crop) drawn on the host, uploaded through a pinned buffer,
    and ``image_crop_resize`` (csrc/image_crop.hip) crops, resizes with the antialiased
    triangle filter, flips and normalises in one launch.
On CPU the same classes run the torch reference implementation of the transform (the oracle of
the tests). Parity with torchvision/PIL itself is unpinned here (neither is importable): the
kernel implements PIL's upsampling filter (bilinear, half-pixel centres) with PIL-style rounding
to uint8, checked against ``F.interpolate(mode="bilinear", align_corners=False)``.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .._native import native

# REF/data_and_toy_model.py:17-20 (CIFAR-10 per-channel mean / std)
CIFAR_MEAN = (0.4914, 0.4822, 0.4465)
CIFAR_STD = (0.2023, 0.1994, 0.2010)


class HostImageDataset:
    """uint8 images ``[n, H, W, C]`` + int64 labels, in host memory."""

    def __init__(self, images, labels):
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(np.ascontiguousarray(images))
        if isinstance(labels, np.ndarray):
            labels = torch.from_numpy(labels.astype(np.int64))
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise TypeError("HostImageDataset expects uint8 [n, H, W, C] images")
        self.images = images.contiguous()
        self.labels = labels.to(torch.int64).contiguous()
        if len(self.images) != len(self.labels):
            raise ValueError("images / labels length mismatch")

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.images[i], self.labels[i]

    @property
    def hwc(self):
        return tuple(self.images.shape[1:])


def cifar_like_uint8(n: int = 50000, hw: int = 32, num_classes: int = 10, seed: int = 0):
    """Synthetic CIFAR-10-layout data (no network): uint8 32x32x3 images whose per-class mean
    colour differs, so a model can learn the labels."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, num_classes, (n,), generator=g)
    base = torch.randint(40, 216, (num_classes, 1, 1, 3), generator=g).float()
    noise = torch.randn(n, hw, hw, 3, generator=g) * 40.0
    img = (base[labels] + noise).clamp_(0, 255).round_().to(torch.uint8)
    return HostImageDataset(img, labels)


CIFAR10_TRAIN_FILES = tuple(f"data_batch_{i}.bin" for i in range(1, 6))
CIFAR10_TEST_FILES = ("test_batch.bin",)
_CIFAR_RECORD = 1 + 3 * 32 * 32  # label byte + R, G, B planes of 32x32, row-major


def _cifar_dir(root: str) -> str:
    """``root`` itself or the ``cifar-10-batches-bin`` directory the binary archive unpacks to
    (torchvision's CIFAR10(root=...) layout, REF/data_and_toy_model.py:31-36)."""
    import os

    for d in (root, os.path.join(root, "cifar-10-batches-bin")):
        if os.path.isfile(os.path.join(d, "test_batch.bin")) or \
                os.path.isfile(os.path.join(d, "data_batch_1.bin")):
            return d
    raise FileNotFoundError(
        f"no CIFAR-10 binary batches (data_batch_1.bin ... / test_batch.bin) under {root!r} or "
        f"{root!r}/cifar-10-batches-bin: there is no download here -- place the binary archive's "
        "files there (the python-pickle archive is not read: loading pickles executes code)")


def load_cifar10_bin(root: str = "./data", train: bool = True) -> HostImageDataset:
    """CIFAR-10 from its binary distribution: every record is 1 label byte followed by 3072
    bytes (R, G, B planes of 32x32). The files are memory-mapped (no pickle, nothing executed)
    and transposed once to the uint8 [n, 32, 32, 3] layout the native prefetcher gathers from
    (150 MB for the training set)."""
    import os

    d = _cifar_dir(root)
    names = CIFAR10_TRAIN_FILES if train else CIFAR10_TEST_FILES
    imgs, labels = [], []
    for name in names:
        path = os.path.join(d, name)
        raw = np.memmap(path, dtype=np.uint8, mode="r")
        if raw.size % _CIFAR_RECORD:
            raise ValueError(f"{path}: {raw.size} bytes is not a whole number of "
                             f"{_CIFAR_RECORD}-byte CIFAR-10 records")
        rec = raw.reshape(-1, _CIFAR_RECORD)
        labels.append(np.asarray(rec[:, 0], dtype=np.int64))
        imgs.append(np.asarray(rec[:, 1:]).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
        del raw, rec
    if not imgs:
        raise FileNotFoundError(f"no CIFAR-10 files in {d}")
    lab = np.concatenate(labels)
    if lab.size and (lab.min() < 0 or lab.max() > 9):
        raise ValueError("CIFAR-10 labels must be in [0, 9]")
    return HostImageDataset(np.ascontiguousarray(np.concatenate(imgs)), lab)


def write_cifar10_bin(path: str, images: torch.Tensor, labels: torch.Tensor) -> None:
    """Write uint8 [n, 32, 32, 3] images + labels in the CIFAR-10 binary record layout (test
    fixtures, and converting other sources to what load_cifar10_bin reads)."""
    x = images.to(torch.uint8).permute(0, 3, 1, 2).reshape(len(images), -1).numpy()
    rec = np.concatenate([labels.to(torch.uint8).numpy().reshape(-1, 1), x], axis=1)
    rec.astype(np.uint8).tofile(path)


def reference_transform(x_u8: torch.Tensor, flip: torch.Tensor | None, size, mean, std,
                        round_u8: bool = True) -> torch.Tensor:
    """torch implementation of image_transform (CPU path and test oracle); [B,H,W,C] uint8 ->
    [B,C,Ho,Wo] float32."""
    x = x_u8.permute(0, 3, 1, 2).float()
    y = F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    if round_u8:
        y = y.round()
    if flip is not None:
        y = torch.where(flip.bool().view(-1, 1, 1, 1), y.flip(-1), y)
    m = torch.tensor(mean, dtype=torch.float32, device=y.device).view(1, -1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=y.device).view(1, -1, 1, 1)
    return (y / 255.0 - m) / s


class ImageTransform:
    """Resize(size) + RandomHorizontalFlip(flip_p) + ToTensor + Normalize(mean, std)."""

    def __init__(self, size=224, flip_p: float = 0.5, mean=CIFAR_MEAN, std=CIFAR_STD,
                 round_u8: bool = True, channels_last: bool = True):
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.flip_p, self.mean, self.std = float(flip_p), tuple(mean), tuple(std)
        self.round_u8, self.channels_last = round_u8, channels_last

    def __call__(self, x_u8: torch.Tensor, flip: torch.Tensor | None) -> torch.Tensor:
        if x_u8.is_cuda:
            return native().image_transform(x_u8, flip if self.flip_p > 0 else None,
                                            self.size[0], self.size[1], list(self.mean),
                                            list(self.std), self.round_u8, self.channels_last)
        y = reference_transform(x_u8, flip if self.flip_p > 0 else None, self.size, self.mean,
                                self.std, self.round_u8)
        return y.contiguous(memory_format=torch.channels_last) if self.channels_last else y


def _norm_size(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def _check_boxes(boxes: torch.Tensor, n: int) -> None:
    if boxes.dtype != torch.int32 or boxes.dim() != 2 or tuple(boxes.shape) != (n, 4):
        raise ValueError(f"boxes must be int32 [{n}, 4] (top, left, h, w)")
    if n and int(boxes[:, 2:].min()) < 1:
        raise ValueError("boxes need h, w >= 1")


def reference_crop_resize(x_u8: torch.Tensor, boxes: torch.Tensor, flip: torch.Tensor | None,
                          size, mean, std, round_u8: bool = True, fill: float = 0.0,
                          out_dtype=torch.float32) -> torch.Tensor:
    """torch implementation of image_crop_resize (the CPU path): pad with ``fill`` as far as
    the boxes reach, slice each sample's box, antialiased bilinear resize, round, flip,
    normalise; [B,H,W,C] uint8 -> [B,C,Ho,Wo] float32, or with ``out_dtype=torch.uint8`` the
    rounded, flipped grey levels as uint8 [B,Ho,Wo,C]."""
    B, H, W, _ = x_u8.shape
    bx = boxes.tolist()
    pt = max([0] + [-t for t, _, _, _ in bx])
    pl = max([0] + [-l for _, l, _, _ in bx])
    pb = max([0] + [t + h - H for t, _, h, _ in bx])
    pr = max([0] + [l + w - W for _, l, _, w in bx])
    x = F.pad(x_u8.permute(0, 3, 1, 2).float(), (pl, pr, pt, pb), value=float(fill))
    y = torch.cat([F.interpolate(x[b:b + 1, :, t + pt:t + pt + h, l + pl:l + pl + w],
                                 size=tuple(size), mode="bilinear", antialias=True,
                                 align_corners=False)
                   for b, (t, l, h, w) in enumerate(bx)]) if B else x.new_empty(0, x.shape[1], *size)
    if round_u8:
        y = y.round()
    if flip is not None:
        y = torch.where(flip.bool().view(-1, 1, 1, 1), y.flip(-1), y)
    if out_dtype == torch.uint8:
        return y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    m = torch.tensor(mean, dtype=torch.float32, device=y.device).view(1, -1, 1, 1)
    s = torch.tensor(std, dtype=torch.float32, device=y.device).view(1, -1, 1, 1)
    return (y / 255.0 - m) / s


def crop_resize(x_u8: torch.Tensor, boxes: torch.Tensor, flip: torch.Tensor | None, size,
                mean, std, round_u8: bool = True, channels_last: bool = True,
                fill: float = 0.0, out_dtype=torch.float32) -> torch.Tensor:
    """Crop sample b of ``x_u8`` [B,H,W,C] to ``boxes[b] = (top, left, h, w)`` (int32; parts
    outside the image read ``fill``), resize the crop to ``size`` with the antialiased triangle
    filter, round like a uint8 image, flip where ``flip[b]``, normalise. On a GPU tensor this is
    the native kernel; host boxes are validated here and uploaded without a sync, device boxes
    are read back once by the binding to validate them.

    ``out_dtype=torch.uint8`` stops after the rounding and the flip and returns the grey levels
    as uint8 [B,Ho,Wo,C], the layout ``augment_batch`` and ``normalize_erase`` read (``mean``,
    ``std`` and ``channels_last`` are ignored; ``round_u8=False`` is an error);
    ``normalize_erase`` of that result is the float32 result bit for bit."""
    return _crop_resize(x_u8, boxes, flip, size, mean, std, round_u8, channels_last, fill,
                        out_dtype, check_device_boxes=True)


def _crop_resize(x_u8, boxes, flip, size, mean, std, round_u8, channels_last, fill, out_dtype,
                 check_device_boxes):
    """crop_resize; ``check_device_boxes=False`` trusts device boxes (no read-back, so the call
    can be captured): the kernel clamps h, w to at least 1."""
    size = _norm_size(size)
    if out_dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"crop_resize: out_dtype must be float32 or uint8 (got {out_dtype})")
    u8 = out_dtype == torch.uint8
    if u8 and not round_u8:
        raise ValueError("crop_resize: a uint8 output is rounded; round_u8=False contradicts it")
    if x_u8.is_cuda:
        host_boxes = not boxes.is_cuda
        if host_boxes:
            _check_boxes(boxes, x_u8.shape[0])
            boxes = boxes.to(x_u8.device, non_blocking=True)
        return native().image_crop_resize(x_u8, boxes, flip, size[0], size[1], list(mean),
                                          list(std), round_u8, channels_last, float(fill),
                                          check_boxes=not host_boxes and check_device_boxes,
                                          out_u8=u8)
    _check_boxes(boxes, x_u8.shape[0])
    y = reference_crop_resize(x_u8, boxes, flip, size, mean, std, round_u8, fill, out_dtype)
    return y if u8 else y.contiguous(memory_format=torch.channels_last) if channels_last else y


def resized_crop_boxes(n: int, H: int, W: int, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
                       generator: torch.Generator | None = None) -> torch.Tensor:
    """RandomResizedCrop's boxes (torchvision's rule), int32 [n, 4] = (top, left, h, w): area
    fraction uniform in ``scale``, aspect ratio log-uniform in ``ratio``, w = round(sqrt(area r)),
    h = round(sqrt(area / r)); of ten tries per sample (one [n, 10] draw) the first that fits the
    image is taken, else the central crop clamped to the ratio bounds; uniform top-left."""
    tries = 10
    u = torch.rand(2, n, tries, generator=generator, dtype=torch.float64)
    pos = torch.rand(n, 2, generator=generator, dtype=torch.float64)
    area = H * W * (scale[0] + (scale[1] - scale[0]) * u[0])
    lr0, lr1 = float(np.log(ratio[0])), float(np.log(ratio[1]))
    r = torch.exp(lr0 + (lr1 - lr0) * u[1])
    w = torch.round(torch.sqrt(area * r)).long()
    h = torch.round(torch.sqrt(area / r)).long()
    ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    first = ok.int().argmax(1, keepdim=True)  # index of the first valid try (0 if none)
    any_ok = ok.any(1)
    w, h = w.gather(1, first).squeeze(1), h.gather(1, first).squeeze(1)
    top = torch.floor(pos[:, 0] * (H - h + 1).clamp(min=1)).long()
    left = torch.floor(pos[:, 1] * (W - w + 1).clamp(min=1)).long()
    # fallback: whole image, cut centrally to the nearest allowed ratio
    if W / H < min(ratio):
        fw, fh = W, int(round(W / min(ratio)))
    elif W / H > max(ratio):
        fh, fw = H, int(round(H * max(ratio)))
    else:
        fw, fh = W, H
    fh, fw = min(max(fh, 1), H), min(max(fw, 1), W)
    fb = torch.tensor([(H - fh) // 2, (W - fw) // 2, fh, fw])
    box = torch.stack([top, left, h, w], 1)
    return torch.where(any_ok.view(-1, 1), box, fb.view(1, 4)).to(torch.int32)


def pad_crop_boxes(n: int, H: int, W: int, size, padding: int,
                   generator: torch.Generator | None = None) -> torch.Tensor:
    """RandomCrop(size, padding)'s boxes: top-left uniform in [-padding, H + padding - size]."""
    sh, sw = _norm_size(size)
    if sh > H + 2 * padding or sw > W + 2 * padding:
        raise ValueError("crop size larger than the padded image")
    top = torch.randint(-padding, H + padding - sh + 1, (n,), generator=generator)
    left = torch.randint(-padding, W + padding - sw + 1, (n,), generator=generator)
    return torch.stack([top, left, torch.full_like(top, sh), torch.full_like(top, sw)],
                       1).to(torch.int32)


def center_crop_boxes(n: int, H: int, W: int, fraction: float = 0.875) -> torch.Tensor:
    """The central ``fraction`` of each side (224 of 256 by default), the usual evaluation crop."""
    h, w = max(1, int(round(H * fraction))), max(1, int(round(W * fraction)))
    return torch.tensor([[(H - h) // 2, (W - w) // 2, h, w]], dtype=torch.int32).repeat(n, 1)


class CropTransform:
    """RandomResizedCrop / RandomCrop(padding) / centre crop to ``size`` +
    RandomHorizontalFlip(flip_p) + ToTensor + Normalize(mean, std); called like ImageTransform.

    The boxes of each batch come from the transform's own CPU generator, which ``start_epoch``
    reseeds (PrefetchLoader does so with its per-(seed, epoch) value), and reach the GPU through
    a pinned buffer and a non-blocking copy: no host sync.

    ``augment`` (e.g. a ``TrivialAugment``: anything with ``draw(n, H, W)`` giving
    ``augment_batch`` params) and ``erase`` (a ``RandomErasing``) switch to torchvision's order:
    the crop kernel writes the uint8 crop, the augmentation runs on that crop (its TranslateX/Y
    pixels and its statistics are the crop's), and ``normalize_erase`` normalises and erases.
    With both ``None`` the transform is the single fused launch. ``apply`` runs the same steps on
    parameters the caller supplies (host or device tensors)."""

    def __init__(self, size=224, crop: str = "random_resized", scale=(0.08, 1.0),
                 ratio=(3 / 4, 4 / 3), padding: int = 4, fraction: float = 0.875,
                 flip_p: float = 0.5, mean=CIFAR_MEAN, std=CIFAR_STD, round_u8: bool = True,
                 channels_last: bool = True, augment=None, erase=None):
        if crop not in ("random_resized", "random_pad", "center"):
            raise ValueError(f"unknown crop {crop!r}")
        if (augment is not None or erase is not None) and not round_u8:
            raise ValueError("CropTransform: augment / erase work on the uint8 crop; "
                             "round_u8=False contradicts it")
        self.augment, self.erase = augment, erase
        self.size, self.crop = _norm_size(size), crop
        self.scale, self.ratio = tuple(scale), tuple(ratio)
        self.padding, self.fraction = int(padding), float(fraction)
        self.flip_p, self.mean, self.std = float(flip_p), tuple(mean), tuple(std)
        self.round_u8, self.channels_last = round_u8, channels_last
        self._gen = torch.Generator().manual_seed(0)

    def start_epoch(self, seed: int) -> None:
        self._gen.manual_seed(int(seed))
        for k, t in enumerate((self.augment, self.erase), 1):
            if hasattr(t, "start_epoch"):
                t.start_epoch(int(seed) + k)

    def boxes(self, n: int, H: int, W: int) -> torch.Tensor:
        if self.crop == "random_resized":
            return resized_crop_boxes(n, H, W, self.scale, self.ratio, self._gen)
        if self.crop == "random_pad":
            return pad_crop_boxes(n, H, W, self.size, self.padding, self._gen)
        return center_crop_boxes(n, H, W, self.fraction)

    def __call__(self, x_u8: torch.Tensor, flip: torch.Tensor | None) -> torch.Tensor:
        n, H, W, _ = x_u8.shape
        boxes = self.boxes(n, H, W)
        if x_u8.is_cuda:
            # torch's pinned-host cache keeps the buffer alive until the copy has run
            boxes = torch.empty_like(boxes, pin_memory=True).copy_(boxes)
        flip = flip if self.flip_p > 0 else None
        if self.augment is None and self.erase is None:
            return crop_resize(x_u8, boxes, flip, self.size, self.mean, self.std, self.round_u8,
                               self.channels_last)
        params = None if self.augment is None else self.augment.draw(n, *self.size)
        eboxes, seed = (None, 0) if self.erase is None else self.erase.draw(n, *self.size)
        return self.apply(x_u8, flip, boxes, params, eboxes, seed)

    def apply(self, x_u8: torch.Tensor, flip: torch.Tensor | None, boxes: torch.Tensor,
              params: torch.Tensor | None = None, erase_boxes: torch.Tensor | None = None,
              seed: int = 0) -> torch.Tensor:
        """Crop to uint8 with ``boxes``, ``augment_batch`` with ``params`` (if given),
        ``normalize_erase`` with ``erase_boxes`` and ``seed``. Host tensors are validated and
        uploaded; device tensors are trusted and nothing is read back, so the call can be
        captured in a graph (where ``seed`` is fixed at capture)."""
        from .augment import augment_batch
        from .erase import normalize_erase

        u8 = _crop_resize(x_u8, boxes, flip, self.size, self.mean, self.std, True,
                          self.channels_last, 0.0, torch.uint8, check_device_boxes=False)
        if params is not None:
            u8 = augment_batch(u8, params)
        return normalize_erase(u8, self.mean, self.std, erase_boxes,
                               0.0 if self.erase is None else self.erase.value, seed,
                               self.channels_last)


def _epoch_seed(seed: int, epoch: int) -> int:
    return (int(seed) * 1000003 + int(epoch) * 7919 + 12345) & 0xFFFFFFFFFFFF


class PrefetchLoader:
    """DataLoader for a HostImageDataset: (inputs, labels) device batches in sampler order.

    ``sampler`` (e.g. DistributedSampler) is re-iterated every epoch, so ``set_epoch`` works as
    with torch's DataLoader; the flip bits change with the sampler's epoch (or with every pass
    when the sampler has none)."""

    def __init__(self, dataset: HostImageDataset, batch_size: int, sampler=None,
                 drop_last: bool = False, transform: ImageTransform | None = None, device=None,
                 depth: int = 4, threads: int = 2, seed: int = 0):
        self.dataset, self.batch_size, self.sampler = dataset, batch_size, sampler
        self.drop_last = drop_last
        self.transform = transform or ImageTransform()
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.seed = seed
        self._passes = 0
        self._native = native().HostBatchLoader(dataset.images.reshape(len(dataset), -1),
                                                dataset.labels, batch_size, depth=depth,
                                                threads=threads,
                                                pinned=self.device.type == "cuda")

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        idx = list(self.sampler) if self.sampler is not None else list(range(len(self.dataset)))
        epoch = getattr(self.sampler, "epoch", None)
        epoch = self._passes if epoch is None else epoch
        self._passes += 1
        self._native.start_epoch(idx, self.drop_last, _epoch_seed(self.seed, epoch),
                                 self.transform.flip_p)
        if hasattr(self.transform, "start_epoch"):
            self.transform.start_epoch(_epoch_seed(self.seed, epoch))
        h, w, c = self.dataset.hwc
        dev = str(self.device)
        while True:
            out = self._native.next(dev)
            if out is None:
                return
            xu8, y, flip = out
            yield self.transform(xu8.view(-1, h, w, c), flip), y
