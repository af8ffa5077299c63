"""The evaluation tail of the reference's sample_50k.py (:174-209, `FID: ..., Inception Score: ...`) and of evaluation/fid.py:8-48 (`get_fid_is`): torch-fidelity's
Frechet Inception Distance against precomputed `mu` / `sigma` statistics and its Inception Score, fed from device memory batch by batch -- by
`SamplePipeline.run(..., metrics=...)` as the images leave the decoder, or from a folder of images written earlier by either side.

What runs where: the uint8 -> f32 resize to the network's input (torch-fidelity's TF1-style bilinear rule, no re-quantisation) and the Inception Score
(f64, fixed-order sums) are HIP kernels of this package (csrc/fidelity.hip); the fake side's f64 feature statistics are `ops.fid_accumulate` and the helpers of
dmvae_amd/fid.py (`mean_cov`, `frechet_distance`).  The split assignment is a pure host function, `row_order`: rows sorted by image index, then permuted by
`np.random.RandomState(rng_seed).permutation(N)`; the kernel takes it as one int64 table.

torch-fidelity is on none of the machines this package was developed on.  The two kernels restate its `interpolate_bilinear_2d_like_tensorflow1x`
(align_corners=False) and `isc_features_to_metric` from their published form (include/dmvae_hip.h gives the definitions, tests/fidelity_spec.py restates them
in numpy); AGREEMENT WITH THE LIBRARY ITSELF HAS NOT BEEN RUN.

Not built here: the Inception network and its weights (`extractor` is the caller's module, as in `fid.FID`), an adapter around torch-fidelity's own extractor
class, a shadow of `get_fid_is` (it needs that network), and torch-fidelity's shuffle of the file list -- the split assignment here depends on the image
indices and `rng_seed` only.

CPU tensors take the stock PyTorch composition behind `DMVAE_ALLOW_STOCK=1`, like every other module (dmvae_amd/_stock.py)."""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _stock, dist, ops
from .fid import frechet_distance, mean_cov

__all__ = ["FidelityMetrics", "InceptionScore", "row_order"]

_IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg")


def row_order(index, shuffle: bool = True, rng_seed: int = 0) -> np.ndarray:
    """index [N] (each row's global image index) -> int64 [N]: position j of the scored sequence holds row `row_order(...)[j]`.  The rows in ascending index
    (a stable sort), then -- when `shuffle` -- permuted by `np.random.RandomState(rng_seed).permutation(N)`.  Pure host function."""
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    order = np.argsort(index, kind="stable").astype(np.int64)
    if shuffle:
        order = order[np.random.RandomState(rng_seed).permutation(len(order))]
    return order


def _stock_resize_tf1_bilinear(u8: torch.Tensor, size: int, nhwc: bool) -> torch.Tensor:
    """The index-select form of the resize on f32 tensors, then (x - 128) / 128: the CPU route."""
    x = (u8.permute(0, 3, 1, 2) if nhwc else u8).float()
    h, w = x.shape[-2:]

    def taps(n_in):
        g = torch.arange(size, dtype=torch.float32) * (n_in / size)
        i0 = g.floor().long()
        return i0, (i0 + 1).clamp(max=n_in - 1), g - i0.float()
    y0, y1, dy = taps(h)
    x0, x1, dx = taps(w)
    dy, dx = dy.view(1, 1, size, 1), dx.view(1, 1, 1, size)
    r0, r1 = x.index_select(2, y0), x.index_select(2, y1)
    a, b, c, d = r0.index_select(3, x0), r0.index_select(3, x1), r1.index_select(3, x0), r1.index_select(3, x1)
    top = a + (b - a) * dx
    bot = c + (d - c) * dx
    return ((top + (bot - top) * dy) - 128) / 128


def _stock_inception_score(logits: torch.Tensor, order: torch.Tensor, splits: int) -> torch.Tensor:
    """The double-softmax loop on f64 tensors: the CPU route."""
    x = logits.double()[order]
    p, logp = x.softmax(dim=1), x.log_softmax(dim=1)
    n, out = x.shape[0], []
    for k in range(splits):
        pk, lk = p[k * n // splits:(k + 1) * n // splits], logp[k * n // splits:(k + 1) * n // splits]
        kl = pk * (lk - pk.mean(dim=0, keepdim=True).log())
        out.append(kl.sum(dim=1).mean().exp())
    return torch.stack(out)


class InceptionScore:
    """The logits of every image seen so far, f32 [N, num_classes] on the device of the first batch (a buffer that doubles when full: 50 000 x 1008 f32 are
    200 MB) with each row's global image index, and the Inception Score of their splits on the HIP kernel.  No host synchronisation before `scores`."""

    def __init__(self, num_classes: int = 1008):
        if not 2 <= int(num_classes) <= 65536:
            raise ValueError(f"InceptionScore: num_classes must lie in [2, 65536] (dmvae_inception_score), got {num_classes}")
        self.num_classes = int(num_classes)
        self.reset()

    def reset(self) -> None:
        self._logits: Optional[torch.Tensor] = None
        self._index: Optional[torch.Tensor] = None
        self._n = 0

    def __len__(self) -> int:
        return self._n

    @property
    def logits(self) -> torch.Tensor:
        """f32 [N, num_classes]: the rows in arrival order (a view of the buffer)."""
        return torch.empty(0, self.num_classes) if self._logits is None else self._logits[:self._n]

    @property
    def index(self) -> torch.Tensor:
        return torch.empty(0, dtype=torch.int64) if self._index is None else self._index[:self._n]

    @torch.no_grad()
    def update_logits(self, logits: torch.Tensor, index: Optional[torch.Tensor] = None) -> None:
        """logits [B, num_classes] (stored as f32); index: int64 [B], each row's global image index (default: arrival order, N .. N + B - 1)."""
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"InceptionScore.update_logits: expected [B, {self.num_classes}], got {tuple(logits.shape)}")
        b = logits.shape[0]
        if b == 0:
            return
        if not logits.is_cuda:
            _stock.require_opt_in("InceptionScore.update_logits", "CPU logits")
        dev = logits.device
        if index is None:
            index = torch.arange(self._n, self._n + b, dtype=torch.int64, device=dev)
        index = torch.as_tensor(index).to(dev, torch.int64).reshape(-1)
        if index.numel() != b:
            raise ValueError(f"InceptionScore.update_logits: {index.numel()} indices for {b} rows")
        if self._logits is not None and self._logits.device != dev:
            raise ValueError(f"InceptionScore.update_logits: logits on {dev}, earlier rows on {self._logits.device}")
        if self._logits is None or self._n + b > self._logits.shape[0]:
            cap = max(self._n + b, 2 * (0 if self._logits is None else self._logits.shape[0]), 64)
            grown = torch.empty(cap, self.num_classes, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
            if self._n:
                grown[0][:self._n].copy_(self._logits[:self._n])
                grown[1][:self._n].copy_(self._index[:self._n])
            self._logits, self._index = grown
        self._logits[self._n:self._n + b].copy_(logits)
        self._index[self._n:self._n + b].copy_(index)
        self._n += b

    def _gathered(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(logits, index) of every rank, rank-major, where dmvae_amd.dist runs more than one (equal counts per rank, as sample_50k.py:137 asserts)."""
        logits, index = self.logits, self.index
        if dist.initialized() and dist.get_world_size() > 1:
            world = dist.get_world_size()
            logits = dist.all_gather_into(torch.empty(world * self._n, self.num_classes, dtype=torch.float32, device=logits.device), logits)
            index = dist.all_gather_into(torch.empty(world * self._n, dtype=torch.int64, device=index.device), index)
        return logits, index

    @torch.no_grad()
    def scores(self, splits: int = 10, shuffle: bool = True, rng_seed: int = 0) -> torch.Tensor:
        """-> f64 [splits] on the logits' device: the score of each split of the rows in `row_order`.  The same value on every rank."""
        logits, index = self._gathered()
        n, splits = logits.shape[0], int(splits)
        if splits < 1 or n < splits:
            raise ValueError(f"InceptionScore.scores: {n} row(s) for {splits} split(s)")
        order = torch.from_numpy(row_order(index.cpu().numpy(), shuffle, rng_seed))
        if logits.is_cuda:
            return ops.inception_score(logits, order.to(logits.device), splits)
        _stock.require_opt_in("InceptionScore.scores", "CPU logits")
        return _stock_inception_score(logits, order, splits)

    def compute(self, splits: int = 10, shuffle: bool = True, rng_seed: int = 0) -> Tuple[float, float]:
        """-> (mean, std) of the splits' scores as Python floats; std is the population form, as np.std."""
        s = self.scores(splits, shuffle, rng_seed).cpu().numpy()
        return float(np.mean(s)), float(np.std(s))


class FidelityMetrics(nn.Module):
    """extractor: a module / callable f32 [B, 3, eval_size, eval_size], normalised as (resize(u8) - 128) / 128, -> (features [B, num_features], logits
    [B, num_classes]).  num_features % 16 == 0, 16 <= num_features <= 4096 (the accumulate kernel's range).
    Buffers: features_sum f64 [F], features_cov_sum f64 [F, F] -- the fake side's statistics, the states of `fid.FID` -- and the host count `num_samples`;
    `isc` is the `InceptionScore`.  Move the object with .to(device) before the first update."""

    def __init__(self, extractor, *, num_features: int, num_classes: int = 1008, eval_size: int = 299):
        super().__init__()
        num_features = int(num_features)
        if num_features % 16 or not 16 <= num_features <= 4096:
            raise ValueError(f"FidelityMetrics: num_features must be a multiple of 16 in [16, 4096] (dmvae_fid_accumulate), got {num_features}")
        if not callable(extractor):
            raise TypeError(f"extractor must be a module / callable, got {type(extractor).__name__}")
        self.extractor, self.num_features, self.eval_size = extractor, num_features, int(eval_size)
        self.isc = InceptionScore(num_classes)
        self.register_buffer("features_sum", torch.zeros(num_features, dtype=torch.float64))
        self.register_buffer("features_cov_sum", torch.zeros(num_features, num_features, dtype=torch.float64))
        self.num_samples = 0
        self.reference: Optional[Tuple[torch.Tensor, torch.Tensor]] = None

    def reset(self) -> None:
        """Clears the accumulated images; loaded reference statistics stay."""
        self.features_sum.zero_()
        self.features_cov_sum.zero_()
        self.num_samples = 0
        self.isc.reset()

    # ---- accumulation ------------------------------------------------------------------------------
    @torch.no_grad()
    def update_uint8(self, images: torch.Tensor, index: Optional[torch.Tensor] = None, nhwc: bool = True) -> None:
        """images uint8 [B, H, W, 3] (nhwc, the layout of `VAE.decode_uint8`) or [B, 3, H, W]; index: int64 [B], the images' global indices (default:
        arrival order).  Resize kernel -> extractor -> both accumulators.  No host synchronisation."""
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise TypeError(f"FidelityMetrics.update_uint8: expected a 4-D uint8 tensor, got {images.dtype} {tuple(images.shape)}")
        if images.shape[0] == 0:
            return
        if images.is_cuda:
            x = ops.resize_tf1_bilinear(images.contiguous(), self.eval_size, nhwc)
        else:
            _stock.require_opt_in("FidelityMetrics.update_uint8", "CPU images")
            x = _stock_resize_tf1_bilinear(images, self.eval_size, nhwc)
        features, logits = self.extractor(x)
        self.update_features(features, logits, index)

    @torch.no_grad()
    def update_features(self, features: torch.Tensor, logits: torch.Tensor, index: Optional[torch.Tensor] = None) -> None:
        """The extractor's outputs of one batch into the two accumulators: features [B, F] (f32, bf16 or f64) in f64, logits [B, num_classes]."""
        if (features.dim() != 2 or features.shape[1] != self.num_features or logits.dim() != 2 or logits.shape[1] != self.isc.num_classes
                or logits.shape[0] != features.shape[0]):
            raise ValueError(f"FidelityMetrics.update_features: expected [B, {self.num_features}] and [B, {self.isc.num_classes}], got "
                             f"{tuple(features.shape)} and {tuple(logits.shape)}")
        if features.dtype not in (torch.float32, torch.bfloat16, torch.float64):
            features = features.float()
        s, c = self.features_sum, self.features_cov_sum
        if features.device != s.device:
            raise ValueError(f"FidelityMetrics.update_features: features on {features.device}, states on {s.device}; move the object with .to(device)")
        self.isc.update_logits(logits, index)
        if features.is_cuda:
            ops.fid_accumulate(features, s, c)
        else:
            _stock.require_opt_in("FidelityMetrics.update_features", "CPU features")
            x = features.double()
            s += x.sum(dim=0)
            c += x.t().mm(x)
        self.num_samples += features.shape[0]

    def update_folder(self, path, batch_size: int = 50) -> int:
        """Every *.png / *.jpg / *.jpeg under `path` (recursively, in sorted order of the paths), decoded to RGB with PIL on the host and fed to `update_uint8`
        in batches of `batch_size` (a batch ends early where the image size changes); the images' indices are their ranks in that order.  -> images read."""
        from PIL import Image
        files = sorted(os.path.join(d, f) for d, _, fs in os.walk(str(path)) for f in fs if f.lower().endswith(_IMAGE_SUFFIXES))
        dev, batch, done = self.features_sum.device, [], 0

        def flush():
            nonlocal batch, done
            if batch:
                self.update_uint8(torch.from_numpy(np.stack(batch)).to(dev), None, nhwc=True)
                done += len(batch)
                batch = []
        for f in files:
            with Image.open(f) as im:
                a = np.asarray(im.convert("RGB"))
            if batch and (a.shape != batch[0].shape or len(batch) == int(batch_size)):
                flush()
            batch.append(a)
        flush()
        return done

    # ---- the values --------------------------------------------------------------------------------
    def load_statistics_file(self, path) -> None:
        """An .npz with `mu` [F] and `sigma` [F, F]: the reference's `fid_statistics_file` (sample_50k.py:174-209), the real side of the FID."""
        with np.load(path) as z:
            mu, sigma = torch.from_numpy(np.asarray(z["mu"], dtype=np.float64)), torch.from_numpy(np.asarray(z["sigma"], dtype=np.float64))
        f = self.num_features
        if tuple(mu.shape) != (f,) or tuple(sigma.shape) != (f, f):
            raise ValueError(f"FidelityMetrics.load_statistics_file: mu {tuple(mu.shape)} / sigma {tuple(sigma.shape)} do not fit {f} features")
        self.reference = (mu, sigma)

    def statistics(self) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """-> (mu f64 [F], sigma f64 [F, F], n) of the images seen so far, on the host, summed over the ranks where dmvae_amd.dist runs more than one (one
        device buffer, one collective, one copy; the states themselves are left alone)."""
        flat = torch.cat([self.features_sum, self.features_cov_sum.reshape(-1),
                          torch.tensor([float(self.num_samples)], dtype=torch.float64, device=self.features_sum.device)])
        if dist.initialized() and dist.get_world_size() > 1:
            dist.allreduce(flat)
        flat, f = flat.cpu(), self.num_features
        n = int(flat[-1].item())
        if n < 2:
            raise RuntimeError(f"FidelityMetrics.statistics: {n} sample(s); a covariance needs two")
        return (*mean_cov(flat[:f], flat[f:f + f * f].view(f, f), n), n)

    def compute(self, splits: int = 10, rng_seed: int = 0) -> Dict[str, float]:
        """-> torch-fidelity's keys: `inception_score_mean`, `inception_score_std`, and -- only when statistics are loaded -- `frechet_inception_distance`."""
        out: Dict[str, float] = {}
        mean, std = self.isc.compute(splits, True, rng_seed)
        out["inception_score_mean"], out["inception_score_std"] = mean, std
        if self.reference is not None:
            mu, sigma, _ = self.statistics()
            out["frechet_inception_distance"] = float(frechet_distance(mu, sigma, *self.reference))
        return out
