"""Device-side input pipeline: what utils/build_dataset.py:55-66 (`train_aug` / `val_aug`) computes per image in PIL, in one HIP pass per batch.

The `DataLoader` workers only decode (`PIL.Image.open(...).convert("RGB")`); `collate_ragged` packs the decoded uint8 HWC images of a batch, at their
own sizes, into one buffer, which the loader's pin thread pins in the main process (`RaggedImages.pin_memory`; a worker never pins and never asks
for the GPU); `DeviceInputPipeline` turns the pack into the `[B, 3, S, S]` float batch (or `[B, S, S, 3]` bytes) that
RandomHorizontalFlip, Resize(mid, LANCZOS), RandomCrop / CenterCrop, ToTensor and `x + x - 1` would have produced -- PIL's bytes, bit for bit
(csrc/data.hip).  Opt-in: nothing else in the package uses it.  JPEG decode stays on the host.

The random draws are made on the host from one generator, per image in the order flip, top, left (the rule is `DeviceInputPipeline.draw`'s own: it
is not checked against torchvision's consumption of its generator); the workers' own random streams are not reproduced and cannot be.  `apply` is deterministic given the draws.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.utils.data

from . import _lib, ops


def _can_pin() -> bool:
    """Pinning allocates through the GPU runtime: only the main process does it.  Inside a DataLoader worker the question is not even put to the runtime
    (a forked child of a process that has initialised the GPU must not touch it); there the loader's pin thread pins the batch in the main process."""
    return torch.utils.data.get_worker_info() is None and torch.cuda.is_available()


def resized_size(w: int, h: int, mid: int) -> Tuple[int, int]:
    """(w', h') of torchvision's Resize(mid) on a w x h image: the shorter edge becomes mid, the longer int(mid * long / short); an image whose shorter
    edge already is mid passes through unchanged."""
    w, h, mid = int(w), int(h), int(mid)
    if w < 1 or h < 1 or mid < 1:
        raise ValueError(f"resized_size: positive sizes required, got w {w}, h {h}, mid {mid}")
    short, long = (w, h) if w <= h else (h, w)
    if short == mid:
        return w, h
    new_long = int(mid * long / short)
    return (mid, new_long) if w <= h else (new_long, mid)


def center_crop_offsets(h: int, w: int, s: int) -> Tuple[int, int]:
    """(top, left) of torchvision's center_crop of an h x w image to s x s: int(round((h - s) / 2.0)), Python's round (half to even)."""
    if s > h or s > w:
        raise ValueError(f"center_crop_offsets: crop {s} larger than the image {h} x {w}")
    return int(round((h - s) / 2.0)), int(round((w - s) / 2.0))


@dataclass
class RaggedImages:
    """A batch of decoded images of different sizes: `data` uint8 1-D, image b is [H, W, 3] RGB at byte `meta[b, 0]`; `meta` [B, 3] int64
    (offset, H, W), always on the host (the tap tables are built from it)."""
    data: torch.Tensor
    meta: torch.Tensor

    def __post_init__(self):
        if self.data.dtype != torch.uint8 or self.data.dim() != 1:
            raise ValueError(f"RaggedImages: data must be a 1-D uint8 tensor, got {self.data.dtype} {tuple(self.data.shape)}")
        if self.meta.dtype != torch.int64 or self.meta.dim() != 2 or self.meta.shape[1] != 3 or self.meta.shape[0] < 1 or self.meta.is_cuda:
            raise ValueError(f"RaggedImages: meta must be a host [B, 3] int64 tensor with B >= 1, got {self.meta.dtype} {tuple(self.meta.shape)}")
        for off, h, w in self.meta.tolist():
            if h < 1 or w < 1 or off < 0 or off + 3 * h * w > self.data.numel():
                raise ValueError(f"RaggedImages: image (offset {off}, {h} x {w}) does not lie inside the {self.data.numel()}-byte pack")

    def __len__(self) -> int:
        return self.meta.shape[0]

    @property
    def device(self) -> torch.device:
        return self.data.device

    def pin_memory(self, device=None) -> "RaggedImages":
        """What `DataLoader(pin_memory=True)`'s pin thread calls on a batch it does not know: the pack in pinned memory (itself when it already is)."""
        return self if self.data.is_pinned() else RaggedImages(self.data.pin_memory(), self.meta)

    def is_pinned(self) -> bool:
        return self.data.is_pinned()

    def to(self, device, non_blocking: bool = False) -> "RaggedImages":
        return RaggedImages(self.data.to(device, non_blocking=non_blocking), self.meta)

    def image(self, b: int) -> torch.Tensor:
        """Image b as a [H, W, 3] view of the pack."""
        off, h, w = self.meta[b].tolist()
        return self.data[off:off + 3 * h * w].view(h, w, 3)


def _as_hwc_u8(img, i: int) -> torch.Tensor:
    if isinstance(img, torch.Tensor):
        t = img
    elif isinstance(img, np.ndarray):
        if img.dtype != np.uint8:
            raise ValueError(f"images[{i}]: expected uint8, got {img.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(img))
    elif hasattr(img, "mode") and hasattr(img, "size") and hasattr(img, "tobytes"):      # a PIL image, without importing PIL
        if img.mode != "RGB":
            raise ValueError(f"images[{i}]: expected a PIL image of mode 'RGB', got {img.mode!r} (decode with .convert('RGB'))")
        t = torch.from_numpy(np.array(img))                         # a copy: PIL's buffer is read-only
    else:
        raise ValueError(f"images[{i}]: expected a PIL image, a numpy array or a tensor, got {type(img).__name__}")
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"images[{i}]: expected uint8 [H, W, 3] (HWC RGB), got {t.dtype} {tuple(t.shape)}")
    return t


def pack_images(images: Sequence) -> RaggedImages:
    """Decoded images (PIL 'RGB' images, numpy arrays or tensors, uint8 [H, W, 3]) -> one uint8 buffer, back to back, and their (offset, H, W).  In
    the main process of a machine with a GPU the buffer is pinned, so that `.to(device, non_blocking=True)` is an asynchronous copy; in a DataLoader worker
    it is ordinary memory and neither pinned memory nor the GPU is asked for (`DataLoader(pin_memory=True)` pins it in the main process)."""
    if len(images) == 0:
        raise ValueError("pack_images: an empty batch")
    ts = [_as_hwc_u8(img, i) for i, img in enumerate(images)]
    meta = torch.empty(len(ts), 3, dtype=torch.int64)
    off = 0
    for i, t in enumerate(ts):
        meta[i, 0], meta[i, 1], meta[i, 2] = off, t.shape[0], t.shape[1]
        off += t.numel()
    data = torch.empty(off, dtype=torch.uint8, pin_memory=_can_pin())
    for i, t in enumerate(ts):
        o = int(meta[i, 0])
        data[o:o + t.numel()].view(t.shape).copy_(t)
    return RaggedImages(data, meta)


def collate_ragged(samples):
    """`collate_fn` of a DataLoader whose dataset yields (decoded image, label): -> (RaggedImages, labels [B] int64)."""
    images, labels = zip(*samples)
    return pack_images(images), torch.as_tensor(labels, dtype=torch.int64)


@functools.lru_cache(maxsize=1024)
def _axis_table(n_in: int, n_out: int, first: int, count: int):
    """One axis' table as dmvae_image_preprocess reads it -- lo [count], n [count], k [count][kmax] in one int32 tensor -- and its kmax.  Cached: the
    coefficients cost two `sin` per tap on the host, and a dataset's common sizes under centre crops (val mode) come back batch after batch."""
    lo, n, k = ops.lanczos_table(n_in, n_out, first, count)
    return torch.cat((lo, n, k.reshape(-1))), k.shape[1]


class DeviceInputPipeline:
    """`train_aug` / `val_aug` of build_dataset(image_size, mode, mid_reso, hflip=...) on a RaggedImages batch.

    draw(ragged) -> (flip [B], top [B], left [B]) int64 host tensors from `generator`: per image `rand(1) < 0.5` (train mode with hflip), then
    `randint(0, H' - S + 1)`, then `randint(0, W' - S + 1)`; no draw where the range is a single value; val mode draws nothing (centre crop, no flip).  This consumption rule is this
    class's own (torchvision's RandomCrop.get_params may draw `randint(0, 1)` on an axis without slack: not checked, torchvision is not a dependency).
    apply(ragged, flip, top, left, out="f32" | "u8") is deterministic; calling the object is apply(ragged, *draw(ragged))."""

    def __init__(self, image_size: int = 256, mid_reso: float = 1.5, mode: str = "train", hflip: bool = True,
                 generator: Optional[torch.Generator] = None):
        if mode not in ("train", "val"):
            raise ValueError(f"mode: expected 'train' or 'val', got {mode!r}")
        self.image_size = int(image_size)
        self.mid = round(mid_reso * self.image_size)            # build_dataset.py:55
        if self.image_size < 1 or self.mid < self.image_size:
            raise ValueError(f"image_size {image_size} with mid_reso {mid_reso}: the resized shorter edge ({self.mid}) must hold the crop")
        self.mode = mode
        self.hflip = bool(hflip)
        self.generator = generator

    def sizes(self, ragged: RaggedImages):
        """[(H', W')] of the batch after Resize(mid)."""
        out = []
        for _, h, w in ragged.meta.tolist():
            w2, h2 = resized_size(w, h, self.mid)
            out.append((h2, w2))
        return out

    def draw(self, ragged: RaggedImages):
        b, s = len(ragged), self.image_size
        flip = torch.zeros(b, dtype=torch.int64)
        top = torch.zeros(b, dtype=torch.int64)
        left = torch.zeros(b, dtype=torch.int64)
        for i, (h2, w2) in enumerate(self.sizes(ragged)):
            if self.mode == "val":
                top[i], left[i] = center_crop_offsets(h2, w2, s)
                continue
            if self.hflip:
                flip[i] = int(torch.rand(1, generator=self.generator).item() < 0.5)
            if h2 - s > 0:
                top[i] = torch.randint(0, h2 - s + 1, (1,), generator=self.generator).item()
            if w2 - s > 0:
                left[i] = torch.randint(0, w2 - s + 1, (1,), generator=self.generator).item()
        return flip, top, left

    def tables(self, ragged: RaggedImages, flip, top, left):
        """The host half of apply: -> (table [B, 12] int64, taps int32 1-D), both on the host (pinned in the main process of a machine with a GPU), as
        dmvae_image_preprocess reads them.  An axis' table is cached by (in, out, first, count): images of one size under the same crop share it."""
        b, s = len(ragged), self.image_size
        flip, top, left = (torch.as_tensor(v, dtype=torch.int64).reshape(-1).tolist() for v in (flip, top, left))
        if not (len(flip) == len(top) == len(left) == b):
            raise ValueError(f"apply: flip, top and left must have one entry per image ({b}), got {len(flip)}, {len(top)}, {len(left)}")
        rows, parts, n_taps = [], [], 0
        for i, ((off, h, w), (h2, w2)) in enumerate(zip(ragged.meta.tolist(), self.sizes(ragged))):
            if not (0 <= top[i] <= h2 - s and 0 <= left[i] <= w2 - s):
                raise ValueError(f"apply: image {i} ({h} x {w} -> {h2} x {w2}): crop corner ({top[i]}, {left[i]}) outside [0, {h2 - s}] x [0, {w2 - s}]")
            if flip[i] not in (0, 1):
                raise ValueError(f"apply: flip[{i}] must be 0 or 1, got {flip[i]}")
            offs, kms = [], []
            for n_in, n_out, first in ((w, w2, left[i]), (h, h2, top[i])):
                if n_in == n_out:                                   # PIL skips a pass whose size does not change
                    offs.append(-1), kms.append(0)
                    continue
                flat, km = _axis_table(n_in, n_out, first, s)
                offs.append(n_taps), kms.append(km)
                parts.append(flat)
                n_taps += flat.numel()
            rows.append([off, h, w, h2, w2, top[i], left[i], flip[i], offs[0], offs[1], kms[0], kms[1]])
        pin = _can_pin()
        rec = torch.tensor(rows, dtype=torch.int64)
        taps = torch.empty(max(n_taps, 1), dtype=torch.int32, pin_memory=pin)
        if parts:
            torch.cat(parts, out=taps[:n_taps])
        else:
            taps.zero_()
        return (rec.pin_memory() if pin else rec), taps

    def apply(self, ragged: RaggedImages, flip, top, left, out: str = "f32", into: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not ragged.data.is_cuda:
            raise _lib.DmvaeHipError("apply: the pack must be on the GPU (ragged.to(device, non_blocking=True)); dmvae_amd has no CPU path")
        rec, taps = self.tables(ragged, flip, top, left)
        dev = ragged.data.device
        return ops.image_preprocess(ragged.data, rec.to(dev, non_blocking=True), taps.to(dev, non_blocking=True), self.image_size, out, into)

    def __call__(self, ragged: RaggedImages, out: str = "f32") -> torch.Tensor:
        return self.apply(ragged, *self.draw(ragged), out=out)
