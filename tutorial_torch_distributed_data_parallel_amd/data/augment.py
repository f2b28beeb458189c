"""TrivialAugmentWide on the uint8 batch (``csrc/image_augment.hip``).

``augment_batch(x_u8, params)`` applies one op per sample to a uint8 ``[N, H, W, C]`` batch
(``C`` in {1, 3}), out of place; ``params`` is int32 ``[N, 8] = (op, a0..a5, 0)``. Every rule is
integer, or fp32 with each operation rounded on its own, so the GPU kernels and
``reference_augment`` (eager torch: the CPU path and the tests' oracle) agree bit for bit.

    trunc8(t)      = clamp(t, 0, 255) truncated toward zero
    blend(a, b, f) = trunc8(f*a + (1 - f)*b), ``1 - f`` in fp32
    gray(p)        = p for C == 1, else trunc8(0.2989 r + 0.587 g + 0.114 b), summed left to right

    0 Identity      a bitwise copy
    1 Affine        a0..a5 = m0..m5, Q16. With u = 2j+1-W, v = 2i+1-H of output pixel (i, j), in
                    int64 U = m0 u + m1 v + m2, V = m3 u + m4 v + m5; the source column is
                    (U + (W<<16)) >> 17, the row (V + (H<<16)) >> 17 (nearest, ties up); a source
                    outside the image gives 0. ShearX/Y, TranslateX/Y and Rotate are this op.
    2 Brightness    a0 = fp32 bits of f: blend(p, 0, f)
    3 Color         blend(p_c, gray(p), f); a copy for C == 1
    4 Contrast      mean = float32(double(sum of gray) / double(H W)): blend(p, mean, f)
    5 Sharpness     interior pixels: T = 3x3 sum + 4 centre, blur = (2T + 13) // 26 (= round(T/13));
                    border pixels: blur = p; blend(p, blur, f); a copy when H < 3 or W < 3
    6 Posterize     a0 = bits in 0..8: p & (0xFF << (8 - bits))
    7 Solarize      a0 = fp32 bits of thr: 255 - p where float(p) >= thr
    8 AutoContrast  per channel lo, hi: trunc8(float(p - lo) * (255.0f / float(hi - lo))), unchanged
                    when hi == lo
    9 Equalize      per channel: step = (H W - hist[last non-empty bin]) // 255; unchanged when 0,
                    else lut[0] = 0, lut[k] = min(255, (hist[0] + .. + hist[k-1] + step//2) // step)

Host ``params`` are validated here and uploaded through a pinned buffer without a sync; device
``params`` are trusted, and the kernel reads an op outside the table as Identity and clamps
``bits``. ``TrivialAugment`` draws torchvision's ``TrivialAugmentWide`` policy per sample and
``AugmentedTransform`` chains it in front of an ``ImageTransform`` / ``CropTransform`` for
``PrefetchLoader``. Unlike torchvision, the augmentation runs on the source image before the
crop and resize, not after: TranslateX/Y's 32 pixels are source pixels.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .._native import native

(IDENTITY, AFFINE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE, SOLARIZE, AUTOCONTRAST,
 EQUALIZE) = range(10)
_BLEND_OPS = (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS)
_STATS_OPS = (CONTRAST, AUTOCONTRAST, EQUALIZE)
_F_MAX = 65536.0  # |f| bound of host params: no blend can overflow fp32


def float_bits(v: float) -> int:
    """The int32 that holds the fp32 bits of ``v`` (how a0 carries ``f`` and ``thr``)."""
    return int(np.float32(v).view(np.int32))


def affine_params(kind: str, value: float, H: int = 0, W: int = 0) -> list:
    """``[m0..m5]`` in Q16 (``round(x * 65536)``), centred coordinates, output -> source:
    ``shear_x`` / ``shear_y`` by the factor ``value``, ``translate_x`` / ``translate_y`` by
    ``value`` source pixels (the image moves right / down), ``rotate`` by ``value`` degrees
    (90 is ``torch.rot90``). ``H`` and ``W`` are not needed by any of them (the kernel centres)."""
    m = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    if kind == "shear_x":
        m[1] = value
    elif kind == "shear_y":
        m[3] = value
    elif kind == "translate_x":
        m[2] = -2.0 * value
    elif kind == "translate_y":
        m[5] = -2.0 * value
    elif kind == "rotate":
        c, s = math.cos(math.radians(value)), math.sin(math.radians(value))
        m = [c, -s, 0.0, s, c, 0.0]
    else:
        raise ValueError(f"affine_params: unknown kind {kind!r}")
    q = [int(round(v * 65536)) for v in m]
    if any(abs(v) >= 2 ** 31 for v in q):
        raise ValueError(f"affine_params: {kind} by {value} does not fit Q16 in int32")
    return q


def make_params(rows) -> torch.Tensor:
    """int32 ``[N, 8]`` from ``(op, a0, a1, ...)`` rows, missing arguments 0."""
    p = torch.zeros(len(rows), 8, dtype=torch.int32)
    for n, r in enumerate(rows):
        p[n, :len(r)] = torch.tensor([int(v) for v in r], dtype=torch.int32)
    return p


def _check(x: torch.Tensor, params: torch.Tensor) -> None:
    if x.dtype != torch.uint8:
        raise TypeError(f"augment_batch: x must be uint8 (got {x.dtype})")
    if params.dtype != torch.int32:
        raise TypeError(f"augment_batch: params must be int32 (got {params.dtype})")
    if x.dim() != 4 or x.shape[3] not in (1, 3):
        raise ValueError(f"augment_batch: x must be [N, H, W, C] with C in (1, 3) "
                         f"(got {tuple(x.shape)})")
    if tuple(params.shape) != (x.shape[0], 8):
        raise ValueError(f"augment_batch: params must be [{x.shape[0]}, 8] "
                         f"(got {tuple(params.shape)})")
    if x.shape[0] > 65535:
        raise ValueError("augment_batch: at most 65535 samples per call")
    if not x.is_contiguous():
        raise ValueError("augment_batch: x must be contiguous")


def _check_host_params(params: torch.Tensor) -> None:
    op, a0 = params[:, 0], params[:, 1]
    if params.shape[0] == 0:
        return
    if int(op.min()) < 0 or int(op.max()) > EQUALIZE:
        raise ValueError("augment_batch: op outside 0..9")
    f = a0.contiguous().view(torch.float32)
    blend = torch.isin(op, torch.tensor(_BLEND_OPS, dtype=torch.int32))
    if bool((blend & ~(f.abs() <= _F_MAX)).any()):
        raise ValueError(f"augment_batch: a blend factor must be finite, |f| <= {_F_MAX:g}")
    if bool(((op == POSTERIZE) & ((a0 < 0) | (a0 > 8))).any()):
        raise ValueError("augment_batch: Posterize bits outside 0..8")
    if bool(((op == SOLARIZE) & f.isnan()).any()):
        raise ValueError("augment_batch: Solarize threshold is NaN")


def _trunc8(t: torch.Tensor) -> torch.Tensor:
    return t.clamp(0, 255).to(torch.uint8)


def _blend(a: torch.Tensor, b, f: torch.Tensor) -> torch.Tensor:
    return _trunc8(f * a + (1 - f) * b)


def _gray(img: torch.Tensor) -> torch.Tensor:
    """uint8 [H, W, C] -> uint8 [H, W]."""
    if img.shape[2] == 1:
        return img[..., 0]
    r, g, b = img.float().unbind(2)
    return _trunc8(0.2989 * r + 0.587 * g + 0.114 * b)


def _affine(img: torch.Tensor, m) -> torch.Tensor:
    H, W, _ = img.shape
    i = torch.arange(H, dtype=torch.int64, device=img.device).view(H, 1)
    j = torch.arange(W, dtype=torch.int64, device=img.device).view(1, W)
    u, v = 2 * j + 1 - W, 2 * i + 1 - H
    sx = (m[0] * u + m[1] * v + m[2] + (W << 16)) >> 17
    sy = (m[3] * u + m[4] * v + m[5] + (H << 16)) >> 17
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    src = img[sy.clamp(0, H - 1), sx.clamp(0, W - 1)]
    return torch.where(ok.unsqueeze(2), src, torch.zeros_like(src))


def _sharpness(img: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    H, W, _ = img.shape
    if H < 3 or W < 3:
        return img.clone()
    p = img.to(torch.int32)
    t = 4 * p[1:-1, 1:-1]
    for di in range(3):
        for dj in range(3):
            t = t + p[di:H - 2 + di, dj:W - 2 + dj]
    blur = p.clone()
    blur[1:-1, 1:-1] = (2 * t + 13) // 26
    return _blend(img.float(), blur.float(), f)


def _autocontrast(img: torch.Tensor) -> torch.Tensor:
    lo = img.amin((0, 1), keepdim=True).to(torch.int32)
    hi = img.amax((0, 1), keepdim=True).to(torch.int32)
    span = hi - lo
    # one rounded division (``255.0 / tensor`` would be reciprocal-then-multiply)
    scale = torch.full_like(span, 255, dtype=torch.float32) / span.clamp(min=1).float()
    out = _trunc8((img.to(torch.int32) - lo).float() * scale)
    return torch.where(span > 0, out, img)


def _equalize(img: torch.Tensor) -> torch.Tensor:
    H, W, C = img.shape
    out = []
    for c in range(C):
        ch = img[..., c].long()
        hist = torch.bincount(ch.reshape(-1), minlength=256)
        last = hist.nonzero().max()
        step = (H * W - hist[last]) // 255
        below = hist.cumsum(0) - hist
        lut = ((below + step // 2) // step.clamp(min=1)).clamp(max=255)
        lut[0] = 0
        lut = torch.where(step > 0, lut, torch.arange(256, device=img.device))
        out.append(lut[ch].to(torch.uint8))
    return torch.stack(out, 2)


def _reference_one(img: torch.Tensor, p: list) -> torch.Tensor:
    op = p[0]
    f = torch.tensor([p[1]], dtype=torch.int32).view(torch.float32).to(img.device)[0]
    if op == AFFINE:
        return _affine(img, p[1:7])
    if op == BRIGHTNESS:
        return _blend(img.float(), 0.0, f)
    if op == COLOR and img.shape[2] == 3:
        return _blend(img.float(), _gray(img).float().unsqueeze(2), f)
    if op == CONTRAST:
        mean = (_gray(img).sum(dtype=torch.int64).double() / float(img.shape[0] * img.shape[1]))
        return _blend(img.float(), mean.float(), f)
    if op == SHARPNESS:
        return _sharpness(img, f)
    if op == POSTERIZE:
        return img & ((0xFF << (8 - p[1])) & 0xFF)
    if op == SOLARIZE:
        return torch.where(img.float() >= f, 255 - img, img)
    if op == AUTOCONTRAST:
        return _autocontrast(img)
    if op == EQUALIZE:
        return _equalize(img)
    return img.clone()


def reference_augment(x_u8: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """The module's rules in eager torch, sample by sample (the CPU path of ``augment_batch`` and
    the oracle of the GPU tests; on GPU tensors it is the composition a user would launch)."""
    _check(x_u8, params)
    params = params.cpu()
    _check_host_params(params)
    rows = params.tolist()
    out = torch.empty_like(x_u8)
    for n, row in enumerate(rows):
        out[n] = _reference_one(x_u8[n], row)
    return out


def augment_batch(x_u8: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """Apply ``params[n]`` to sample ``n`` of ``x_u8`` (see the module text). On a GPU batch this is
    two launches (statistics, apply) and no sync; the statistics launch is skipped when host
    ``params`` hold no Contrast, AutoContrast or Equalize."""
    _check(x_u8, params)
    if not x_u8.is_cuda:
        return reference_augment(x_u8, params)
    stats = True
    if not params.is_cuda:
        _check_host_params(params)
        stats = bool(torch.isin(params[:, 0], torch.tensor(_STATS_OPS, dtype=torch.int32)).any())
        if not params.is_pinned():
            # torch's pinned-host cache keeps the buffer alive until the copy has run
            params = torch.empty(params.shape, dtype=torch.int32, pin_memory=True).copy_(params)
        params = params.to(x_u8.device, non_blocking=True)
    params = params.contiguous()
    C = native()
    return C.image_augment_apply(x_u8, params,
                                 C.image_augment_stats(x_u8, params) if stats else None)


# torchvision's TrivialAugmentWide op space: (name, largest magnitude, signed)
_TA_OPS = (("Identity", 0.0, False), ("ShearX", 0.99, True), ("ShearY", 0.99, True),
           ("TranslateX", 32.0, True), ("TranslateY", 32.0, True), ("Rotate", 135.0, True),
           ("Brightness", 0.99, True), ("Color", 0.99, True), ("Contrast", 0.99, True),
           ("Sharpness", 0.99, True), ("Posterize", 0.0, False), ("Solarize", 255.0, False),
           ("AutoContrast", 0.0, False), ("Equalize", 0.0, False))
_TA_AFFINE = {"ShearX": "shear_x", "ShearY": "shear_y", "TranslateX": "translate_x",
              "TranslateY": "translate_y", "Rotate": "rotate"}
_TA_BLEND = {"Brightness": BRIGHTNESS, "Color": COLOR, "Contrast": CONTRAST,
             "Sharpness": SHARPNESS}


class TrivialAugment:
    """torchvision's ``TrivialAugmentWide`` for a uint8 batch: per sample one of 14 ops, uniform,
    at a uniform bin of ``num_bins``; magnitude ``linspace(0, max, num_bins)[bin]`` with ``max``
    0.99 for ShearX/Y and for Brightness / Color / Contrast / Sharpness (``f = 1 + m``), 32 pixels
    for TranslateX/Y, 135 degrees for Rotate, negated with probability 1/2; Posterize keeps
    ``8 - round(bin / ((num_bins - 1) / 6))`` bits, Solarize takes
    ``linspace(255, 0, num_bins)[bin]``.

    Draws come from the transform's own CPU generator, which ``start_epoch`` reseeds (as
    ``CropTransform``); ``draw(n)`` returns the int32 ``[n, 8]`` params and ``__call__`` applies
    them with ``augment_batch``. The ops act on the source image: used in front of a crop
    (``AugmentedTransform``), TranslateX/Y's 32 pixels are source pixels."""

    op_names = tuple(name for name, _, _ in _TA_OPS)

    def __init__(self, num_bins: int = 31):
        if num_bins < 2:
            raise ValueError("TrivialAugment: num_bins must be >= 2")
        self.num_bins = int(num_bins)
        self._rng = np.random.default_rng(0)

    def start_epoch(self, seed: int) -> None:
        self._rng = np.random.default_rng(int(seed))

    def draw(self, n: int, H: int = 0, W: int = 0) -> torch.Tensor:
        rng, nb = self._rng, self.num_bins
        ops, bins = rng.integers(len(_TA_OPS), size=n), rng.integers(nb, size=n)
        neg = rng.random(n) < 0.5
        rows = []
        for o, b, s in zip(ops.tolist(), bins.tolist(), neg.tolist()):
            name, top, signed = _TA_OPS[o]
            mag = top * b / (nb - 1)
            if signed and s:
                mag = -mag
            if name in _TA_AFFINE:
                rows.append([AFFINE] + affine_params(_TA_AFFINE[name], mag, H, W))
            elif name in _TA_BLEND:
                rows.append([_TA_BLEND[name], float_bits(1.0 + mag)])
            elif name == "Posterize":
                rows.append([POSTERIZE, 8 - int(round(b / ((nb - 1) / 6)))])
            elif name == "Solarize":
                rows.append([SOLARIZE, float_bits(255.0 - mag)])
            else:
                rows.append([{"AutoContrast": AUTOCONTRAST, "Equalize": EQUALIZE}.get(name,
                                                                                     IDENTITY)])
        return make_params(rows)

    def __call__(self, x_u8: torch.Tensor) -> torch.Tensor:
        n, H, W, _ = x_u8.shape
        return augment_batch(x_u8, self.draw(n, H, W))


class AugmentedTransform:
    """``augment`` on the uint8 source batch, then ``transform`` (an ``ImageTransform`` or
    ``CropTransform``); called like them, so ``PrefetchLoader`` takes it unchanged. The
    augmentation sees the source image, before the crop and resize (torchvision applies it after
    the crop)."""

    def __init__(self, augment, transform):
        self.augment, self.transform = augment, transform

    @property
    def flip_p(self) -> float:
        return self.transform.flip_p

    def start_epoch(self, seed: int) -> None:
        for t in (self.augment, self.transform):
            if hasattr(t, "start_epoch"):
                t.start_epoch(seed)

    def __call__(self, x_u8: torch.Tensor, flip: torch.Tensor | None) -> torch.Tensor:
        return self.transform(self.augment(x_u8), flip)
