"""ToTensor + Normalize + RandomErasing on the uint8 batch (``csrc/image_finish.hip``).

``normalize_erase(x_u8, mean, std, boxes)`` turns a uint8 ``[N, H, W, C]`` batch (``C`` in
{1, 3, 4}) into the normalised float32 ``[N, C, H, W]`` batch and erases ``boxes[n] = (top, left,
h, w)`` of sample ``n`` (int32 ``[N, 4]``; ``h == 0`` or ``w == 0``: nothing) in the same launch.
It is the step after the uint8 crop (``crop_resize(out_dtype=torch.uint8)``) and the uint8
augmentation, which is torchvision's order: crop, flip, TrivialAugment, ToTensor, Normalize,
RandomErasing.

Per element ``(n, c, i, j)``:

    outside the box   fma(x, 1/255, -mean[c]) * (1 / std[c]) in fp32, the crop kernel's expression:
                      without boxes, ``normalize_erase(crop_resize(..., out_dtype=torch.uint8))``
                      equals ``crop_resize(...)`` bit for bit
    inside, a float or C floats   that value as given; it is not normalised (torchvision erases
                      after Normalize; its default is 0)
    inside, "random"  a standard normal per element (torchvision's ``value="random"``, timm's
                      ``pixel`` mode). With e = (c*H + i)*W + j, Philox4x32-10 under the key
                      (seed & 0xFFFFFFFF, seed >> 32) maps the counter (e >> 2, 0, n, 0) to four
                      32-bit words, of which word e & 3 is u1; the same word for the counter
                      (e >> 2, 0, n, 1) is u2, and
                          z = sqrt(-2 log((u1 + 1) * 2^-32)) * cos(6.2831855 * (u2 * 2^-32)),
                      every operation one rounded fp32 operation. z depends on (seed, n, c, i, j)
                      only: not on the layout, the launch grid or the batch around the sample
                      (``sample_offset`` is added to n, so a sample run alone can reproduce it).

``seed`` is a host integer passed by value: inside a captured graph it is fixed at capture, as
for ``ops.dropout``. Host ``boxes`` are validated (they must lie inside the image) and uploaded
through a pinned buffer without a sync; device ``boxes`` are trusted, and the kernel clamps them to
the image. One box per sample, fp32 output only. ``reference_normalize_erase`` is the same rule in
eager torch: the CPU path and the tests' oracle.
"""
from __future__ import annotations

import numpy as np
import torch

from .._native import native

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF
TWO_PI_F32 = float(np.float32(2.0 * np.pi))  # 6.2831855, the rule's constant


def _mulhilo(m: int, x: torch.Tensor):
    """(high, low) 32 bits of m * x for 32-bit x held in int64, without leaving int64."""
    hi = (m * (x >> 16) + ((m * (x & 0xFFFF)) >> 16)) >> 16
    return hi, (m * x) & _MASK


def _philox(c0, c1, c2, c3, k0: int, k1: int):
    for _ in range(10):
        h0, l0 = _mulhilo(_M0, c0)
        h1, l1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return torch.stack([c0, c1, c2, c3])


def philox_uniforms(seed: int, N: int, C: int, H: int, W: int, sample_offset: int = 0,
                    device="cpu"):
    """The exact 32-bit integers (u1, u2) of the "random" rule, int64 ``[N, C, H, W]`` each."""
    e = torch.arange(C * H * W, dtype=torch.int64, device=device).view(1, C, H, W)
    q = (e >> 2).expand(N, C, H, W)
    n = (torch.arange(N, dtype=torch.int64, device=device) + int(sample_offset)).view(N, 1, 1, 1)
    n, zero = n.expand_as(q), torch.zeros_like(q)
    k0, k1 = int(seed) & _MASK, (int(seed) >> 32) & _MASK
    lane = (e & 3).expand(1, N, C, H, W)
    u = [_philox(q & _MASK, q >> 32, n, zero + w, k0, k1).gather(0, lane)[0] for w in (0, 1)]
    return u[0], u[1]


def normal_from_uniforms(u1: torch.Tensor, u2: torch.Tensor, dtype=torch.float32):
    """The rule's z from (u1, u2) with every operation in ``dtype`` (float64: the tests' truth)."""
    a = (u1.to(dtype) + 1) * 2.0 ** -32
    return torch.sqrt(-2 * torch.log(a)) * torch.cos(TWO_PI_F32 * (u2.to(dtype) * 2.0 ** -32))


def _check(x: torch.Tensor) -> None:
    if x.dtype != torch.uint8:
        raise TypeError(f"normalize_erase: x must be uint8 (got {x.dtype})")
    if x.dim() != 4 or x.shape[3] not in (1, 3, 4):
        raise ValueError(f"normalize_erase: x must be [N, H, W, C] with C in (1, 3, 4) "
                         f"(got {tuple(x.shape)})")
    if x.shape[0] > 65535:
        raise ValueError("normalize_erase: at most 65535 samples per call")
    if not x.is_contiguous():
        raise ValueError("normalize_erase: x must be contiguous")


def _check_host_boxes(boxes: torch.Tensor, N: int, H: int, W: int) -> None:
    if boxes.dtype != torch.int32 or tuple(boxes.shape) != (N, 4):
        raise ValueError(f"normalize_erase: boxes must be int32 [{N}, 4] (top, left, h, w)")
    if N == 0:
        return
    t, l, h, w = boxes.long().unbind(1)
    if bool(((h < 0) | (w < 0)).any()):
        raise ValueError("normalize_erase: boxes need h, w >= 0")
    live = (h > 0) & (w > 0)
    if bool((live & ((t < 0) | (l < 0) | (t + h > H) | (l + w > W))).any()):
        raise ValueError(f"normalize_erase: a box reaches outside the {H} x {W} image")


def _fill(value, C: int):
    """(mode, C floats) of ``value``: a float, C floats or "random"."""
    if isinstance(value, str):
        if value != "random":
            raise ValueError(f"normalize_erase: unknown value {value!r}")
        return 1, [0.0] * C
    vals = [float(v) for v in value] if isinstance(value, (tuple, list)) else [float(value)] * C
    if len(vals) != C:
        raise ValueError(f"normalize_erase: value needs {C} floats (got {len(vals)})")
    return 0, vals


def reference_normalize_erase(x_u8: torch.Tensor, mean, std, boxes=None, value=0.0, seed: int = 0,
                              sample_offset: int = 0) -> torch.Tensor:
    """``normalize_erase`` in eager torch, [N, C, H, W] float32 (plain contiguous), bit for bit the
    kernel's constant modes. The kernel's fused multiply-add is a 256-entry table per channel
    evaluated in float64 and rounded once, which is exact for mean[c] == 0 or |mean[c]| >= 2^-21
    (the product has 32 significant bits). Boxes are clamped to the image as the kernel does."""
    _check(x_u8)
    N, H, W, C = x_u8.shape
    dev = x_u8.device
    mode, vals = _fill(value, C)
    k = torch.tensor(1.0, dtype=torch.float32) / 255.0
    m = torch.tensor(list(mean), dtype=torch.float32).double().view(C, 1)
    inv = (1.0 / torch.tensor(list(std), dtype=torch.float64)).float().view(C, 1)
    lut = ((torch.arange(256, dtype=torch.float64) * k.double() - m).float() * inv).to(dev)
    y = lut[torch.arange(C, device=dev).view(1, C, 1, 1), x_u8.permute(0, 3, 1, 2).long()]
    if boxes is None:
        return y
    inside = torch.zeros(N, 1, H, W, dtype=torch.bool)
    for n, (t, l, h, w) in enumerate(boxes.cpu().tolist()):
        if h > 0 and w > 0:
            inside[n, :, max(t, 0):min(t + h, H), max(l, 0):min(l + w, W)] = True
    if mode == 1:
        fill = normal_from_uniforms(*philox_uniforms(seed, N, C, H, W, sample_offset, dev))
    else:
        fill = torch.tensor(vals, dtype=torch.float32, device=dev).view(1, C, 1, 1)
    return torch.where(inside.to(dev), fill, y)


def normalize_erase(x_u8: torch.Tensor, mean, std, boxes=None, value=0.0, seed: int = 0,
                    channels_last: bool = True, sample_offset: int = 0) -> torch.Tensor:
    """uint8 ``[N, H, W, C]`` -> normalised float32 ``[N, C, H, W]`` with ``boxes[n]`` erased to
    ``value`` (a float, C floats, or "random"); see the module text. One launch on a GPU batch.
    ``seed`` is passed by value, so a captured graph replays the seed it was captured with."""
    _check(x_u8)
    N, H, W, C = x_u8.shape
    mode, vals = _fill(value, C)
    if len(mean) != C or len(std) != C:
        raise ValueError(f"normalize_erase: mean / std need {C} values")
    if boxes is not None and not boxes.is_cuda:
        _check_host_boxes(boxes, N, H, W)
    if not x_u8.is_cuda:
        y = reference_normalize_erase(x_u8, mean, std, boxes, value, seed, sample_offset)
        return y.contiguous(memory_format=torch.channels_last) if channels_last else y
    if boxes is not None:
        if not boxes.is_cuda:
            if not boxes.is_pinned():
                # torch's pinned-host cache keeps the buffer alive until the copy has run
                boxes = torch.empty(boxes.shape, dtype=torch.int32, pin_memory=True).copy_(boxes)
            boxes = boxes.to(x_u8.device, non_blocking=True)
        boxes = boxes.contiguous()
    return native().image_normalize_erase(x_u8, boxes, list(mean), list(std), vals, mode,
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset),
                                          channels_last)


def erase_boxes(n: int, H: int, W: int, p: float = 0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3),
                generator: torch.Generator | None = None) -> torch.Tensor:
    """RandomErasing's boxes (torchvision's rule), int32 [n, 4] = (top, left, h, w): a sample is
    erased with probability ``p``; area fraction uniform in ``scale``, aspect ratio log-uniform in
    ``ratio``, h = round(sqrt(area r)), w = round(sqrt(area / r)); of ten tries per sample (one
    [n, 10] draw) the first with 0 < h < H and 0 < w < W is taken, with a uniform top-left corner.
    A sample that is not erased, or for which no try fits, gets the zero box."""
    tries = 10
    keep = torch.rand(n, generator=generator, dtype=torch.float64) < p
    u = torch.rand(2, n, tries, generator=generator, dtype=torch.float64)
    pos = torch.rand(n, 2, generator=generator, dtype=torch.float64)
    area = H * W * (scale[0] + (scale[1] - scale[0]) * u[0])
    lr0, lr1 = float(np.log(ratio[0])), float(np.log(ratio[1]))
    r = torch.exp(lr0 + (lr1 - lr0) * u[1])
    h = torch.round(torch.sqrt(area * r)).long()
    w = torch.round(torch.sqrt(area / r)).long()
    ok = (h > 0) & (h < H) & (w > 0) & (w < W)
    first = ok.int().argmax(1, keepdim=True)  # index of the first valid try (0 if none)
    h, w = h.gather(1, first).squeeze(1), w.gather(1, first).squeeze(1)
    top = torch.floor(pos[:, 0] * (H - h + 1).clamp(min=1)).long()
    left = torch.floor(pos[:, 1] * (W - w + 1).clamp(min=1)).long()
    box = torch.stack([top, left, h, w], 1)
    return torch.where((keep & ok.any(1)).view(-1, 1), box, torch.zeros_like(box)).to(torch.int32)


class RandomErasing:
    """torchvision's ``RandomErasing(p, scale, ratio, value)`` for a batch: ``draw(n, H, W)``
    returns the boxes of ``erase_boxes`` and the batch's kernel seed (used by ``value="random"``),
    both from the transform's own CPU generator, which ``start_epoch`` reseeds (as
    ``CropTransform``); ``__call__`` applies them with ``normalize_erase``."""

    def __init__(self, p: float = 0.1, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0.0):
        if not 0.0 <= p <= 1.0:
            raise ValueError("RandomErasing: p must be in [0, 1]")
        self.p, self.scale, self.ratio, self.value = float(p), tuple(scale), tuple(ratio), value
        self._gen = torch.Generator().manual_seed(0)

    def start_epoch(self, seed: int) -> None:
        self._gen.manual_seed(int(seed))

    def draw(self, n: int, H: int, W: int):
        boxes = erase_boxes(n, H, W, self.p, self.scale, self.ratio, self._gen)
        return boxes, int(torch.randint(0, 2 ** 62, (), generator=self._gen))

    def __call__(self, x_u8: torch.Tensor, mean, std, channels_last: bool = True) -> torch.Tensor:
        n, H, W, _ = x_u8.shape
        boxes, seed = self.draw(n, H, W)
        return normalize_erase(x_u8, mean, std, boxes, self.value, seed, channels_last)
