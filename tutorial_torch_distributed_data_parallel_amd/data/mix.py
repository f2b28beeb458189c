"""MixUp and CutMix on the device batch (``csrc/mix.hip``).

``mix_batch`` is the kernel: for float32 ``x`` ``[N, C, H, W]`` (contiguous or channels_last), a
partner ``perm[b]``, a weight ``lam[b]`` and a box ``boxes[b] = (top, left, h, w)`` per sample,

    out[b, :, i, j] = x[perm[b]]                                 inside the box
                      x[b]                                       outside it, lam[b] == 1
                      lam[b] x[b] + (1 - lam[b]) x[perm[b]]      outside it otherwise

MixUp is an empty box, CutMix is ``lam == 1`` with a real box, and one launch serves a batch that
holds both. It is out of place (a partner may come earlier in the batch), every pure-copy element
is bitwise its source, and it has no backward: mixing is an input transform.

``BatchMix`` draws what ``mix_batch`` needs the way timm's ``Mixup`` and the torchvision
reference recipe do -- one mode, one ``lam`` and one box per batch -- and returns the labels as
the pair ``(ya, yb, lam)`` that ``ops.cross_entropy_pair`` reads.
"""
from __future__ import annotations

import numpy as np
import torch

from .._native import native


def _check(x, perm, lam, boxes):
    if x.dim() != 4:
        raise ValueError(f"mix_batch: x must be [N, C, H, W] (got {x.dim()}-D)")
    n = x.shape[0]
    if perm.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"mix_batch: perm must be int32 or int64 (got {perm.dtype})")
    if lam.dtype != torch.float32:
        raise TypeError(f"mix_batch: lam must be float32 (got {lam.dtype})")
    if boxes.dtype != torch.int32:
        raise TypeError(f"mix_batch: boxes must be int32 (got {boxes.dtype})")
    if tuple(perm.shape) != (n,) or tuple(lam.shape) != (n,) or tuple(boxes.shape) != (n, 4):
        raise ValueError(f"mix_batch: perm and lam must be [{n}], boxes [{n}, 4] "
                         f"(top, left, h, w)")
    if x.requires_grad:
        raise ValueError("mix_batch: x requires grad; mixing is an input transform and has no "
                         "backward")


def reference_mix(x: torch.Tensor, perm: torch.Tensor, lam: torch.Tensor,
                  boxes: torch.Tensor) -> torch.Tensor:
    """The plain torch composition of ``mix_batch`` (the CPU path)."""
    n, _, H, W = x.shape
    xp = x[perm.long()]
    lamv = lam.to(x.dtype).view(n, 1, 1, 1)
    out = torch.where(lamv == 1, x, lamv * x + (1 - lamv) * xp)
    i = torch.arange(H, device=x.device).view(1, H, 1)
    j = torch.arange(W, device=x.device).view(1, 1, W)
    b = boxes.long()
    top, left = b[:, 0].view(n, 1, 1), b[:, 1].view(n, 1, 1)
    inside = ((i >= top) & (i < top + b[:, 2].view(n, 1, 1)) &
              (j >= left) & (j < left + b[:, 3].view(n, 1, 1)))
    return torch.where(inside.unsqueeze(1), xp, out).contiguous(
        memory_format=torch.channels_last if not x.is_contiguous() else torch.contiguous_format)


def mix_batch(x: torch.Tensor, perm: torch.Tensor, lam: torch.Tensor,
              boxes: torch.Tensor) -> torch.Tensor:
    """Mix sample ``b`` of ``x`` with sample ``perm[b]`` (see the module text). ``perm`` int32 or
    int64 ``[N]``, ``lam`` float32 ``[N]``, ``boxes`` int32 ``[N, 4]``; host tensors are checked
    here (``perm`` in range) and uploaded without a sync, device tensors are trusted: the kernel
    clips boxes to the image and reads an out-of-range partner as the sample itself."""
    _check(x, perm, lam, boxes)
    if not x.is_cuda:
        return reference_mix(x, perm, lam, boxes)
    if x.dtype != torch.float32:
        raise TypeError(f"mix_batch: the native kernel is float32 only (got {x.dtype})")
    if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError("mix_batch: x must be contiguous or channels_last")
    if not perm.is_cuda and x.shape[0] and not (0 <= int(perm.min()) and
                                                int(perm.max()) < x.shape[0]):
        raise ValueError("mix_batch: perm out of range")
    perm, lam, boxes = (t if t.is_cuda else t.to(x.device, non_blocking=True)
                        for t in (perm, lam, boxes))
    return native().mix_batch(x, perm.contiguous(), lam.contiguous(), boxes.contiguous())


class BatchMix:
    """MixUp / CutMix for a device batch: ``x_mixed, (ya, yb, lam) = mix(x, y)``, then
    ``ops.cross_entropy_pair(model(x_mixed), ya, yb, lam)``.

    Per batch (timm ``Mixup(mode="batch")``, the torchvision reference recipe): with probability
    ``prob`` the batch is mixed, by CutMix with probability ``switch_prob`` when both alphas are
    positive (else by whichever is); ``lam ~ Beta(alpha, alpha)``; the partner of sample ``b`` is
    ``perm[b]`` of a uniform permutation; CutMix cuts a box of area fraction ``1 - lam`` around a
    uniform centre, clips it to the image and corrects ``lam`` to ``1 - area / (H W)``.

    Everything is drawn on the host from the transform's own generator, which ``start_epoch``
    reseeds (as ``CropTransform``), and reaches the GPU through one pinned buffer and one
    non-blocking copy: no host sync."""

    def __init__(self, mixup_alpha: float = 0.2, cutmix_alpha: float = 1.0, prob: float = 1.0,
                 switch_prob: float = 0.5):
        if mixup_alpha < 0 or cutmix_alpha < 0 or not 0 <= prob <= 1 or not 0 <= switch_prob <= 1:
            raise ValueError("BatchMix: alphas must be >= 0, prob and switch_prob in [0, 1]")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self._rng = np.random.default_rng(0)

    def start_epoch(self, seed: int) -> None:
        self._rng = np.random.default_rng(int(seed))

    def draw(self, n: int, H: int, W: int):
        """One batch's draw on the host: ``(perm int32 [n], lam of the image mix float32 [n],
        boxes int32 [n, 4], lam of the labels float32 [n])``, views of one int32 buffer."""
        return _views(self._draw(n, H, W), n)

    def _draw(self, n: int, H: int, W: int) -> torch.Tensor:
        rng = self._rng
        # every variate is drawn every time, so the stream does not depend on the outcome
        u_on, u_mode = rng.random(), rng.random()
        perm = rng.permutation(n)
        cy, cx = int(rng.integers(H)), int(rng.integers(W))
        cutmix = self.cutmix_alpha > 0 and (self.mixup_alpha == 0 or u_mode < self.switch_prob)
        alpha = self.cutmix_alpha if cutmix else self.mixup_alpha
        lam = float(rng.beta(alpha, alpha)) if alpha > 0 else 1.0
        box = (0, 0, 0, 0)
        if u_on >= self.prob or alpha == 0:
            lam_x = lam_y = 1.0
        elif cutmix:
            r = np.sqrt(1.0 - lam)
            ch, cw = int(H * r), int(W * r)
            t, b = np.clip((cy - ch // 2, cy + ch // 2), 0, H)
            l, rr = np.clip((cx - cw // 2, cx + cw // 2), 0, W)
            box = (int(t), int(l), int(b - t), int(rr - l))
            lam_x, lam_y = 1.0, 1.0 - box[2] * box[3] / (H * W)
        else:
            lam_x = lam_y = lam
        buf = np.empty(7 * n, dtype=np.int32)
        buf[:n] = perm
        buf[n:2 * n] = np.float32(lam_x).view(np.int32)
        buf[2 * n:3 * n] = np.float32(lam_y).view(np.int32)
        buf[3 * n:].reshape(n, 4)[:] = np.asarray(box, dtype=np.int32)
        return torch.from_numpy(buf)

    def __call__(self, x: torch.Tensor, y: torch.Tensor):
        n, _, H, W = x.shape
        buf = self._draw(n, H, W)
        if x.is_cuda:
            # torch's pinned-host cache keeps the buffer alive until the copy has run
            buf = torch.empty_like(buf, pin_memory=True).copy_(buf).to(x.device,
                                                                       non_blocking=True)
        perm, lam_x, boxes, lam_y = _views(buf, n)
        return mix_batch(x, perm, lam_x, boxes), (y, y.index_select(0, perm), lam_y)


def _views(buf: torch.Tensor, n: int):
    """``perm | lam_x | lam_y | boxes`` of BatchMix's flat int32 ``[7 n]`` buffer."""
    return (buf[:n], buf[n:2 * n].view(torch.float32), buf[3 * n:].view(n, 4),
            buf[2 * n:3 * n].view(torch.float32))
