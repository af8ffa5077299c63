"""The evaluation tail of the reference's sample_50k.py (:174-209, `FID: ..., Inception Score: ...`) and of evaluation/fid.py:8-48 (`get_fid_is`): torch-fidelity's
Frechet Inception Distance against precomputed `mu` / `sigma` statistics and its Inception Score, fed from device memory batch by batch -- by
`SamplePipeline.run(..., metrics=...)` as the images leave the decoder, or from a folder of images written earlier by either side -- and the two all-pairs
metrics the same call spells out (sample_50k.py:185-199, evaluation/fid.py:15-45): `kid` (Kernel Inception Distance over random subsets) and `prc`
(precision / recall of the two feature manifolds), on request, from the features kept in a `FeatureBank`.

What runs where: the uint8 -> f32 resize to the network's input (torch-fidelity's TF1-style bilinear rule, no re-quantisation) and the Inception Score
(f64, fixed-order sums) are HIP kernels of this package (csrc/fidelity.hip); the fake side's f64 feature statistics are `ops.fid_accumulate` and the helpers of
dmvae_amd/fid.py (`mean_cov`, `frechet_distance`).  The split assignment is a pure host function, `row_order`: rows sorted by image index, then permuted by
`np.random.RandomState(rng_seed).permutation(N)`; the kernel takes it as one int64 table.  KID and precision / recall are `ops.kid_mmd2`, `ops.knn_radius` and
`ops.manifold_member` (csrc/manifold.hip): f64 Gram tiles with streaming epilogues, nothing N x N in memory, reruns bit-identical; KID's subsets are drawn by
the pure host function `kid_subset_tables`.

torch-fidelity is on none of the machines this package was developed on.  The kernels restate its `interpolate_bilinear_2d_like_tensorflow1x`
(align_corners=False), `isc_features_to_metric`, `polynomial_mmd` (unbiased estimate) and `calc_cdist_part(...).kthvalue(k + 1)` / `(dist <= radii).any(1)`
from their published form (include/dmvae_hip.h gives the definitions, tests/fidelity_spec.py and tests/manifold_spec.py restate them in numpy); AGREEMENT
WITH THE LIBRARY ITSELF HAS NOT BEEN RUN, for the two all-pairs definitions as for the first two.

The Inception network is `dmvae_amd.models.inception.InceptionV3Compat` (`FidelityMetrics(net.extractor(), num_features=2048)`); `extractor` may be any
other module with its contract.  Not here: the network's weight file, an adapter around torch-fidelity's own extractor
class, a shadow of `get_fid_is` (it needs that weight file), `ppl`, and torch-fidelity's shuffle of the file list -- the split assignment and KID's subsets
here depend on the image indices and `rng_seed` only.

CPU tensors take the stock PyTorch composition behind `DMVAE_ALLOW_STOCK=1`, like every other module (dmvae_amd/_stock.py)."""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _stock, dist, ops
from .fid import accumulate_features, check_feature_width, frechet_distance, mean_cov, summed_on_host

__all__ = ["FeatureBank", "FidelityMetrics", "InceptionScore", "kid_subset_tables", "row_order"]

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


class _RowBank:
    """The f32 rows of every batch seen so far, [N, width] on the device of the first batch, with each row's global image index (int64 [N]): a pair of
    buffers that doubles when full.  What `InceptionScore` keeps of the logits and `FeatureBank` of the features; `what` is their name for the rows.
    No host synchronisation in `update`."""

    def __init__(self, width: int, what: str):
        self.width, self._what = int(width), what
        self.reset()

    def reset(self) -> None:
        self._rows: Optional[torch.Tensor] = None
        self._index: Optional[torch.Tensor] = None
        self._n = 0

    def __len__(self) -> int:
        return self._n

    def _apply(self, fn) -> None:
        """The device `FidelityMetrics.to(...)` moves its buffers to, for the rows; their dtypes stay f32 / int64 whatever else `fn` converts."""
        if self._rows is not None:
            dev = fn(self._rows[:0]).device
            self._rows, self._index = self._rows.to(dev), self._index.to(dev)

    @property
    def device(self) -> Optional[torch.device]:
        return None if self._rows is None else self._rows.device

    @property
    def rows(self) -> torch.Tensor:
        """f32 [N, width]: the rows in arrival order (a view of the buffer)."""
        return torch.empty(0, self.width) if self._rows is None else self._rows[:self._n]

    @property
    def index(self) -> torch.Tensor:
        return torch.empty(0, dtype=torch.int64) if self._index is None else self._index[:self._n]

    @torch.no_grad()
    def update(self, rows: torch.Tensor, index: Optional[torch.Tensor], who: str) -> None:
        """rows [B, width] (stored as f32); index: int64 [B], each row's global image index (default: arrival order, N .. N + B - 1).  `who`: the public
        method the messages name."""
        if rows.dim() != 2 or rows.shape[1] != self.width:
            raise ValueError(f"{who}: expected [B, {self.width}], got {tuple(rows.shape)}")
        b = rows.shape[0]
        if b == 0:
            return
        if not rows.is_cuda:
            _stock.require_opt_in(who, f"CPU {self._what}")
        dev = rows.device
        if index is None:
            index = torch.arange(self._n, self._n + b, dtype=torch.int64, device=dev)
        index = torch.as_tensor(index).to(dev, torch.int64).reshape(-1)
        if index.numel() != b:
            raise ValueError(f"{who}: {index.numel()} indices for {b} rows")
        if self._rows is not None and self._rows.device != dev:
            raise ValueError(f"{who}: {self._what} on {dev}, earlier rows on {self._rows.device}")
        if self._rows is None or self._n + b > self._rows.shape[0]:
            cap = max(self._n + b, 2 * (0 if self._rows is None else self._rows.shape[0]), 64)
            grown = torch.empty(cap, self.width, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
            if self._n:
                grown[0][:self._n].copy_(self._rows[:self._n])
                grown[1][:self._n].copy_(self._index[:self._n])
            self._rows, self._index = grown
        self._rows[self._n:self._n + b].copy_(rows)
        self._index[self._n:self._n + b].copy_(index)
        self._n += b

    def gathered(self, skip: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(rows, index) of every rank, rank-major, where dmvae_amd.dist runs more than one (equal counts per rank, as sample_50k.py:137 asserts); `skip`:
        this rank's rows as they are."""
        rows, index = self.rows, self.index
        if not skip and dist.initialized() and dist.get_world_size() > 1:
            world = dist.get_world_size()
            rows = dist.all_gather_into(torch.empty(world * self._n, self.width, dtype=torch.float32, device=rows.device), rows)
            index = dist.all_gather_into(torch.empty(world * self._n, dtype=torch.int64, device=index.device), index)
        return rows, index


class InceptionScore:
    """The logits of every image seen so far, f32 [N, num_classes] on the device of the first batch (a buffer that doubles when full: 50 000 x 1008 f32 are
    200 MB) with each row's global image index, and the Inception Score of their splits on the HIP kernel.  No host synchronisation before `scores`."""

    def __init__(self, num_classes: int = 1008):
        if not 2 <= int(num_classes) <= 65536:
            raise ValueError(f"InceptionScore: num_classes must lie in [2, 65536] (dmvae_inception_score), got {num_classes}")
        self.num_classes = int(num_classes)
        self._bank = _RowBank(self.num_classes, "logits")

    def reset(self) -> None:
        self._bank.reset()

    def __len__(self) -> int:
        return len(self._bank)

    @property
    def logits(self) -> torch.Tensor:
        """f32 [N, num_classes]: the rows in arrival order (a view of the buffer)."""
        return self._bank.rows

    @property
    def index(self) -> torch.Tensor:
        return self._bank.index

    def update_logits(self, logits: torch.Tensor, index: Optional[torch.Tensor] = None) -> None:
        """logits [B, num_classes] (stored as f32); index: int64 [B], each row's global image index (default: arrival order, N .. N + B - 1)."""
        self._bank.update(logits, index, "InceptionScore.update_logits")

    @torch.no_grad()
    def scores(self, splits: int = 10, shuffle: bool = True, rng_seed: int = 0) -> torch.Tensor:
        """-> f64 [splits] on the logits' device: the score of each split of the rows in `row_order`.  The same value on every rank."""
        logits, index = self._bank.gathered()
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


def kid_subset_tables(n1: int, n2: int, subsets: int = 100, subset_size: int = 1000, rng_seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """-> (int64 [subsets, subset_size], int64 [subsets, subset_size]): the positions KID's subsets take in the two feature sequences, by torch-fidelity's
    draws -- one `np.random.RandomState(rng_seed)`, and per subset `choice(n1, subset_size, replace=False)`, then `choice(n2, subset_size, replace=False)`.
    The positions count the rows in ascending image index (`row_order(index, shuffle=False)`); torch-fidelity's shuffled file order is NOT reproduced, as for
    the Inception Score's splits: the subsets depend on the image indices and `rng_seed` only.  Pure host function."""
    n1, n2, subsets, m = int(n1), int(n2), int(subsets), int(subset_size)
    if subsets < 1 or m < 2:
        raise ValueError(f"kid_subset_tables: subsets >= 1 and subset_size >= 2 required, got {subsets} and {m}")
    if m > min(n1, n2):
        raise ValueError(f"kid_subset_tables: subset_size {m} exceeds the smaller feature set ({n1} and {n2} rows)")
    rng = np.random.RandomState(rng_seed)
    t1, t2 = np.empty((subsets, m), dtype=np.int64), np.empty((subsets, m), dtype=np.int64)
    for s in range(subsets):
        t1[s] = rng.choice(n1, m, replace=False)
        t2[s] = rng.choice(n2, m, replace=False)
    return t1, t2


def _stock_dist2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    a, b = a.double(), b.double()
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * a.mm(b.t())).clamp_(min=0)


def _stock_knn_radius(x: torch.Tensor, k: int) -> torch.Tensor:
    """The full f64 distance matrix with its diagonal set to 0, then kthvalue(k + 1): the CPU route."""
    d = _stock_dist2(x, x)
    d.fill_diagonal_(0)
    return d.kthvalue(int(k) + 1, dim=1).values


def _stock_manifold_member(q: torch.Tensor, r: torch.Tensor, radius2: torch.Tensor) -> torch.Tensor:
    return (_stock_dist2(q, r) <= radius2[None, :]).any(dim=1).to(torch.uint8)


def _stock_kid_mmd2(x: torch.Tensor, y: torch.Tensor, idx1: torch.Tensor, idx2: torch.Tensor, degree: int, gamma: Optional[float], coef0: float) -> torch.Tensor:
    """The three kernel matrices of each subset on f64 tensors, the diagonal left out by position: the CPU route."""
    gamma = 1.0 / x.shape[1] if gamma is None else float(gamma)
    out = []
    for i1, i2 in zip(idx1, idx2):
        a, b = x[i1].double(), y[i2].double()
        m = a.shape[0]
        off = ~torch.eye(m, dtype=torch.bool)

        def kern(u, v):
            base = gamma * u.mm(v.t()) + coef0
            p = base
            for _ in range(int(degree) - 1):
                p = p * base
            return p
        out.append((kern(a, a)[off].sum() + kern(b, b)[off].sum()) / (m * (m - 1)) - 2 * kern(a, b).sum() / (m * m))
    return torch.stack(out)


class FeatureBank(_RowBank):
    """The f32 features of every image seen so far, [N, num_features] on the device of the first batch (a buffer that doubles when full: 50 000 x 2048 f32
    are 410 MB), with each row's global image index: what KID and precision / recall need of either side.  No host synchronisation in `update`.
    Where dmvae_amd.dist runs more than one rank, a bank fed by `update` holds THIS RANK'S SHARD (the ranks' rows are gathered when the values are computed),
    a bank filled by `load` holds the WHOLE set on every rank (`is_global`; it is never gathered, and takes no further `update`).  `save` writes the whole
    set.  An image index that occurs twice among the rows that meet -- one file's rows fed as shards on every rank, default indices on several ranks -- is
    refused when the values are computed."""

    def __init__(self, num_features: int):
        super().__init__(check_feature_width(num_features, "FeatureBank: num_features"), "features")

    @property
    def num_features(self) -> int:
        return self.width

    @property
    def features(self) -> torch.Tensor:
        """f32 [N, num_features]: the rows in arrival order (a view of the buffer)."""
        return self.rows

    def reset(self) -> None:
        super().reset()
        self.is_global = False

    def update(self, features: torch.Tensor, index: Optional[torch.Tensor] = None) -> None:
        """features [B, num_features] (stored as f32); index: int64 [B], each row's global image index (default: arrival order, N .. N + B - 1)."""
        if self.is_global:
            raise ValueError("FeatureBank.update: this bank was loaded from a file and holds the whole set on every rank; reset() it before feeding shards")
        super().update(features, index, "FeatureBank.update")

    def save(self, path) -> None:
        """An .npz with `features` f32 [N, num_features] and `index` int64 [N]: the WHOLE set -- every rank's rows, rank-major (a collective where
        dmvae_amd.dist runs more than one rank: every rank calls, rank 0 writes) -- which is what `load` expects."""
        features, index = self.gathered(self.is_global)
        if not (dist.initialized() and dist.get_world_size() > 1) or dist.get_rank() == 0:
            np.savez(path, features=features.cpu().numpy(), index=index.cpu().numpy())

    def load(self, path, device=None) -> None:
        """Replaces the rows by those of an .npz written by `save` (on `device`; default: where the rows were, else the CPU).  The file is the WHOLE set:
        every rank loads all of it, the bank is marked `is_global` and is not gathered over the ranks."""
        with np.load(path) as z:
            features, index = np.asarray(z["features"], dtype=np.float32), np.asarray(z["index"], dtype=np.int64)
        if features.ndim != 2 or features.shape[1] != self.num_features or index.shape != (features.shape[0],):
            raise ValueError(f"FeatureBank.load: features {features.shape} / index {index.shape} do not fit {self.num_features} features")
        dev = device if device is not None else (self.device or "cpu")
        self.reset()
        self.update(torch.from_numpy(features).to(dev), torch.from_numpy(index))
        self.is_global = True

    def ordered(self) -> Tuple[torch.Tensor, np.ndarray]:
        """-> (the gathered features, int64 [N] host table): position j of the sequence in ascending image index is row table[j].  An image index that
        occurs twice is refused: the same rows were fed on several ranks (or without indices on several ranks), and every radius and subset would be wrong."""
        features, index = self.gathered(self.is_global)       # a bank loaded from a file already holds every rank's rows
        index = index.cpu().numpy()
        order = row_order(index, shuffle=False)
        if len(order) > 1 and (np.diff(index[order]) == 0).any():
            raise ValueError(f"FeatureBank: an image index occurs more than once among the {len(order)} rows of all ranks; feed each rank its own shard with "
                             "its images' global indices, or load() the whole set from a file")
        return features, order


class FidelityMetrics(nn.Module):
    """extractor: a module / callable f32 [B, 3, eval_size, eval_size], normalised as (resize(u8) - 128) / 128, -> (features [B, num_features], logits
    [B, num_classes]).  num_features % 16 == 0, 16 <= num_features <= 4096 (the accumulate kernel's range).
    Buffers: features_sum f64 [F], features_cov_sum f64 [F, F] -- the fake side's statistics, the states of `fid.FID` -- and the host count `num_samples`;
    `isc` is the `InceptionScore`.  Move the object with .to(device) before the first update.
    keep_features=True: `update_features` also feeds `bank`, a `FeatureBank` of the fake side (50 000 x 2048 f32: 410 MB of device memory), which
    `compute(kid=True)` / `compute(prc=True)` need next to the real side's `reference_bank` (`update_reference_features`, `update_reference_uint8`,
    `load_reference_features`).  With False (the default) `bank` is None and nothing is allocated."""

    def __init__(self, extractor, *, num_features: int, num_classes: int = 1008, eval_size: int = 299, keep_features: bool = False):
        super().__init__()
        num_features = check_feature_width(num_features, "FidelityMetrics: num_features")
        if not callable(extractor):
            raise TypeError(f"extractor must be a module / callable, got {type(extractor).__name__}")
        self.extractor, self.num_features, self.eval_size = extractor, num_features, int(eval_size)
        self.isc = InceptionScore(num_classes)
        self.register_buffer("features_sum", torch.zeros(num_features, dtype=torch.float64))
        self.register_buffer("features_cov_sum", torch.zeros(num_features, num_features, dtype=torch.float64))
        self.num_samples = 0
        self.reference: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self.bank: Optional[FeatureBank] = FeatureBank(num_features) if keep_features else None
        self.reference_bank: Optional[FeatureBank] = None

    def _apply(self, fn, *args, **kwargs):
        """.to(device) / .cuda() / .cpu() move the two feature banks with the buffers."""
        super()._apply(fn, *args, **kwargs)
        for bank in (getattr(self, "bank", None), getattr(self, "reference_bank", None)):
            if bank is not None:
                bank._apply(fn)
        return self

    def reset(self) -> None:
        """Clears the accumulated images; loaded reference statistics and reference features stay."""
        self.features_sum.zero_()
        self.features_cov_sum.zero_()
        self.num_samples = 0
        self.isc.reset()
        if self.bank is not None:
            self.bank.reset()

    # ---- accumulation ------------------------------------------------------------------------------
    def _resized(self, images: torch.Tensor, nhwc: bool, who: str) -> Optional[torch.Tensor]:
        """uint8 images -> the extractor's f32 input [B, 3, eval_size, eval_size] (None for an empty batch): the resize kernel, or its stock form on the CPU."""
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise TypeError(f"{who}: expected a 4-D uint8 tensor, got {images.dtype} {tuple(images.shape)}")
        if images.shape[0] == 0:
            return None
        if images.is_cuda:
            return ops.resize_tf1_bilinear(images.contiguous(), self.eval_size, nhwc)
        _stock.require_opt_in(who, "CPU images")
        return _stock_resize_tf1_bilinear(images, self.eval_size, nhwc)

    @torch.no_grad()
    def update_uint8(self, images: torch.Tensor, index: Optional[torch.Tensor] = None, nhwc: bool = True) -> None:
        """images uint8 [B, H, W, 3] (nhwc, the layout of `VAE.decode_uint8`) or [B, 3, H, W]; index: int64 [B], the images' global indices (default:
        arrival order).  Resize kernel -> extractor -> both accumulators.  No host synchronisation."""
        x = self._resized(images, nhwc, "FidelityMetrics.update_uint8")
        if x is not None:
            self.update_features(*self.extractor(x), index)

    @torch.no_grad()
    def update_features(self, features: torch.Tensor, logits: torch.Tensor, index: Optional[torch.Tensor] = None) -> None:
        """The extractor's outputs of one batch into the two accumulators: features [B, F] (f32, bf16 or f64) in f64, logits [B, num_classes]."""
        if (features.dim() != 2 or features.shape[1] != self.num_features or logits.dim() != 2 or logits.shape[1] != self.isc.num_classes
                or logits.shape[0] != features.shape[0]):
            raise ValueError(f"FidelityMetrics.update_features: expected [B, {self.num_features}] and [B, {self.isc.num_classes}], got "
                             f"{tuple(features.shape)} and {tuple(logits.shape)}")
        if features.device != self.features_sum.device:       # stricter than accumulate_features: the logits and the bank stay where the features are
            raise ValueError(f"FidelityMetrics.update_features: features on {features.device}, states on {self.features_sum.device}; move the object "
                             "with .to(device)")
        self.isc.update_logits(logits, index)
        self.num_samples += accumulate_features(features, self.features_sum, self.features_cov_sum, "FidelityMetrics.update_features")
        if self.bank is not None:
            self.bank.update(features, index)

    # ---- the real side's features (KID, precision / recall) ---------------------------------------
    @torch.no_grad()
    def update_reference_features(self, features: torch.Tensor, index: Optional[torch.Tensor] = None) -> None:
        """The extractor's features of one batch of REAL images [B, F] into `reference_bank` (made on first use); the fake side's states are not touched."""
        if features.dim() != 2 or features.shape[1] != self.num_features:
            raise ValueError(f"FidelityMetrics.update_reference_features: expected [B, {self.num_features}], got {tuple(features.shape)}")
        if self.reference_bank is None:
            self.reference_bank = FeatureBank(self.num_features)
        self.reference_bank.update(features, index)

    @torch.no_grad()
    def update_reference_uint8(self, images: torch.Tensor, index: Optional[torch.Tensor] = None, nhwc: bool = True) -> None:
        """REAL images, as `update_uint8` takes the sampled ones: resize kernel -> extractor -> `reference_bank`.  No effect on the fake side's states."""
        x = self._resized(images, nhwc, "FidelityMetrics.update_reference_uint8")
        if x is not None:
            self.update_reference_features(self.extractor(x)[0], index)

    def load_reference_features(self, path) -> None:
        """An .npz written by `FeatureBank.save` (`features` [N, F], `index` [N]) as the real side, on the device of the states.  The file is the WHOLE real
        set: with more than one rank every rank loads all of it and it is not gathered (only the fake side, fed per rank, is)."""
        bank = FeatureBank(self.num_features)
        bank.load(path, device=self.features_sum.device)
        self.reference_bank = bank

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
        s, c, n = summed_on_host([self.features_sum, self.features_cov_sum,
                                  torch.tensor(float(self.num_samples), dtype=torch.float64, device=self.features_sum.device)])
        n = int(n.item())
        if n < 2:
            raise RuntimeError(f"FidelityMetrics.statistics: {n} sample(s); a covariance needs two")
        return (*mean_cov(s, c, n), n)

    def _banks(self, what: str) -> Tuple[FeatureBank, FeatureBank]:
        if self.bank is None:
            raise RuntimeError(f"FidelityMetrics.compute({what}=True): no fake-side features were kept; build the object with keep_features=True")
        if self.reference_bank is None or len(self.reference_bank) == 0:
            raise RuntimeError(f"FidelityMetrics.compute({what}=True): no real-side features; feed update_reference_uint8 / update_reference_features or "
                               "call load_reference_features")
        if len(self.bank) == 0:
            raise RuntimeError(f"FidelityMetrics.compute({what}=True): no fake-side features yet")
        if self.bank.device != self.reference_bank.device:
            raise RuntimeError(f"FidelityMetrics.compute({what}=True): fake-side features on {self.bank.device}, real-side features on "
                               f"{self.reference_bank.device}; move the object with .to(device)")
        return self.bank, self.reference_bank

    def kid_values(self, subsets: int = 100, subset_size: int = 1000, degree: int = 3, gamma: Optional[float] = None, coef0: float = 1.0,
                   rng_seed: int = 0) -> torch.Tensor:
        """-> f64 [subsets] on the features' device: the unbiased polynomial MMD^2 of each of `kid_subset_tables`' subsets, fake side first."""
        fake, real = self._banks("kid")
        (x, o1), (y, o2) = fake.ordered(), real.ordered()
        t1, t2 = kid_subset_tables(len(o1), len(o2), subsets, subset_size, rng_seed)
        idx1, idx2 = torch.from_numpy(o1[t1]), torch.from_numpy(o2[t2])
        if x.is_cuda:
            return ops.kid_mmd2(x, y, idx1.to(x.device), idx2.to(x.device), degree, gamma, coef0)
        _stock.require_opt_in("FidelityMetrics.kid_values", "CPU features")
        return _stock_kid_mmd2(x, y, idx1, idx2, degree, gamma, coef0)

    def precision_recall(self, neighborhood: int = 3) -> Tuple[float, float]:
        """-> (precision, recall): the share of fake rows inside some real row's ball of radius its `neighborhood`-th neighbour, and of real rows inside
        some fake row's."""
        fake, real = self._banks("prc")
        x, y = fake.ordered()[0], real.ordered()[0]                  # the rows as gathered (their order does not matter here); duplicate indices refused
        if x.is_cuda:
            inside_real = ops.manifold_member(x, y, ops.knn_radius(y, neighborhood))
            inside_fake = ops.manifold_member(y, x, ops.knn_radius(x, neighborhood))
        else:
            _stock.require_opt_in("FidelityMetrics.precision_recall", "CPU features")
            inside_real = _stock_manifold_member(x, y, _stock_knn_radius(y, neighborhood))
            inside_fake = _stock_manifold_member(y, x, _stock_knn_radius(x, neighborhood))
        return float(inside_real.double().mean().item()), float(inside_fake.double().mean().item())

    def compute(self, splits: int = 10, rng_seed: int = 0, *, kid: bool = False, prc: bool = False, kid_subsets: int = 100, kid_subset_size: int = 1000,
                kid_degree: int = 3, kid_gamma: Optional[float] = None, kid_coef0: float = 1.0, prc_neighborhood: int = 3) -> Dict[str, float]:
        """-> torch-fidelity's keys: `inception_score_mean`, `inception_score_std`, and -- only when statistics are loaded -- `frechet_inception_distance`.
        kid=True adds `kernel_inception_distance_mean` / `_std` (np.mean / np.std of the f64 subset values), prc=True adds `precision`, `recall` and
        `f_score` = 2 p r / max(p + r, 1e-5); both need the two feature banks and raise RuntimeError without them."""
        out: Dict[str, float] = {}
        for flag, what in ((kid, "kid"), (prc, "prc")):
            if flag:
                self._banks(what)                                     # a missing bank is an error before anything is computed, never a skipped key
        mean, std = self.isc.compute(splits, True, rng_seed)
        out["inception_score_mean"], out["inception_score_std"] = mean, std
        if self.reference is not None:
            mu, sigma, _ = self.statistics()
            out["frechet_inception_distance"] = float(frechet_distance(mu, sigma, *self.reference))
        if kid:
            v = self.kid_values(kid_subsets, kid_subset_size, kid_degree, kid_gamma, kid_coef0, rng_seed).cpu().numpy()
            out["kernel_inception_distance_mean"], out["kernel_inception_distance_std"] = float(np.mean(v)), float(np.std(v))
        if prc:
            p, r = self.precision_recall(prc_neighborhood)
            out["precision"], out["recall"] = p, r
            out["f_score"] = float(2 * p * r / max(p + r, 1e-5))
        return out
