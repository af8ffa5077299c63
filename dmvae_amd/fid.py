"""FID around a pluggable feature extractor: the reference's `evaluation.fid.FID` (evaluation/fid.py:51-95, a torchmetrics FrechetInceptionDistance with a
bicubic resize and the uint8 quantisation in front) with the same protocol -- `update(images01, real)`, `compute()`, `reset()`, `save` / `load` -- and the same
state layout, so that statistics files written by either side load in the other.

What runs where: the resize + quantisation (evaluation/fid.py:61-64) and the f64 feature statistics `sum += X.sum(0)`, `cov_sum += X^T X` (torchmetrics'
`update`) are HIP kernels of this package (csrc/fid.hip: no ATen interpolate, no vendor GEMM).  `feature` is either a module mapping uint8 [B, 3, S, S] to
[B, F] -- the package's own Inception network is `dmvae_amd.models.inception.InceptionV3Compat` (`FID(feature=InceptionV3Compat.from_checkpoint(path))`;
the weight file is not shipped) -- or the int that asks torchmetrics for its `NoTrainInceptionV3` (an ImportError without torchmetrics).  `compute()` runs
once per evaluation, in f64 on the host: mean and covariance from the
sums, then `frechet_distance` through `torch.linalg.eigvals`.

CPU tensors take the stock PyTorch composition behind `DMVAE_ALLOW_STOCK=1`, like every other module (dmvae_amd/_stock.py)."""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _stock, dist, ops

__all__ = ["FID", "frechet_distance", "mean_cov"]

_SIDES = ("fake", "real")


def frechet_distance(mu1: torch.Tensor, sigma1: torch.Tensor, mu2: torch.Tensor, sigma2: torch.Tensor) -> torch.Tensor:
    """|mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 sum Re sqrt(eigvals(sigma1 sigma2)), in f64 on the host -> 0-d f64 tensor (torchmetrics'
    `_compute_fid`: the trace of the matrix square root is the sum of the square roots of the product's eigenvalues)."""
    mu1, sigma1, mu2, sigma2 = (torch.as_tensor(t).detach().to("cpu", torch.float64) for t in (mu1, sigma1, mu2, sigma2))
    d = mu1 - mu2
    ev = torch.linalg.eigvals(sigma1 @ sigma2)
    return d.dot(d) + sigma1.trace() + sigma2.trace() - 2 * ev.sqrt().real.sum()


def mean_cov(s: torch.Tensor, cov_sum: torch.Tensor, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The states of n samples -> (mean = sum / n, cov = (cov_sum - n mean mean^T) / (n - 1)), as torchmetrics' `compute` forms them."""
    mu = s / n
    return mu, (cov_sum - n * torch.outer(mu, mu)) / (n - 1)


def check_feature_width(num, who: str) -> int:
    """F % 16 == 0, 16 <= F <= 4096: the range of the accumulate kernel (dmvae_fid_accumulate) and of the Gram tiles (csrc/manifold.hip) -> int(num).
    `who` names the object and its argument: "FID: the feature width", "FeatureBank: num_features"."""
    num = int(num)
    if num % 16 or not 16 <= num <= 4096:
        raise ValueError(f"{who} must be a multiple of 16 in [16, 4096], got {num}")
    return num


def accumulate_features(features: torch.Tensor, s: torch.Tensor, c: torch.Tensor, who: str) -> int:
    """One batch of features [B, F] (or [F]: one row) into the f64 states, s [F] += X.sum(0), c [F, F] += X^T X -> B.  f32, bf16 and f64 go in as they are,
    anything else as f32.  GPU features need the states on their device and run `ops.fid_accumulate`; CPU features take the stock route behind
    DMVAE_ALLOW_STOCK=1, on the states' device.  An empty batch changes nothing.  `who` is the public method the messages name."""
    if features.dim() == 1:
        features = features.unsqueeze(0)
    if features.dim() != 2 or features.shape[1] != s.shape[0]:
        raise ValueError(f"{who}: expected [B, {s.shape[0]}], got {tuple(features.shape)}")
    if features.dtype not in (torch.float32, torch.bfloat16, torch.float64):
        features = features.float()
    if features.shape[0] == 0:
        return 0
    if features.is_cuda:
        if features.device != s.device:
            raise ValueError(f"{who}: features on {features.device}, states on {s.device}; move the object with .to(device)")
        ops.fid_accumulate(features, s, c)
    else:
        _stock.require_opt_in(who, "CPU features")
        x = features.double().to(s.device)
        s += x.sum(dim=0)
        c += x.t().mm(x)
    return features.shape[0]


def summed_on_host(states):
    """A list of state tensors of one device -> the same list in f64 on the host, summed over the ranks where dmvae_amd.dist runs more than one: one flat
    device buffer (the states themselves are left alone, so a second call counts nothing twice), one collective, one copy.  Counts are exact in f64 below 2^53."""
    flat = torch.cat([t.to(torch.float64).reshape(-1) for t in states])
    if dist.initialized() and dist.get_world_size() > 1:
        dist.allreduce(flat)
    return [part.view(t.shape) for part, t in zip(flat.cpu().split([t.numel() for t in states]), states)]


def _stock_resize_u8(imgs: torch.Tensor, size: int) -> torch.Tensor:
    """evaluation/fid.py:61-64 as written: the CPU route."""
    if imgs.size(-1) != size or imgs.size(-2) != size:
        imgs = F.interpolate(imgs, size=(size, size), mode="bicubic")
    return (imgs * 255).clamp(0, 255).to(dtype=torch.uint8)


class FID(nn.Module):
    """feature: a module / callable uint8 [B, 3, eval_size, eval_size] -> [B, F] (F from its `num_features`, else from one probe call on a zero image), or an
    int: torchmetrics' NoTrainInceptionV3 at that feature width.  F % 16 == 0, 16 <= F <= 4096 (the accumulate kernel's range).
    normalize: only False, the reference's default, which its trainers use (images in [0, 1] are quantised here, evaluation/fid.py:63-64).
    Buffers, with the reference's names and dtypes: {real,fake}_features_sum f64 [F], {real,fake}_features_cov_sum f64 [F, F],
    {real,fake}_features_num_samples int64 scalars."""

    def __init__(self, feature=2048, eval_size: int = 299, normalize: bool = False, *, reset_real_features: bool = True):
        super().__init__()
        if normalize:
            raise ValueError("FID(normalize=True) is not built: the resize kernel quantises with the clamp of evaluation/fid.py:64, torchmetrics' own "
                             "`(imgs * 255).byte()` wraps; the reference's trainers pass normalize=False")
        self.eval_size, self.normalize, self.reset_real_features = int(eval_size), False, bool(reset_real_features)
        if isinstance(feature, bool) or not (isinstance(feature, int) or callable(feature)):
            raise TypeError(f"feature must be an int or a module / callable, got {type(feature).__name__}")
        if isinstance(feature, int):
            try:
                from torchmetrics.image.fid import NoTrainInceptionV3
            except ImportError as e:
                raise ImportError(f"FID(feature={feature}) builds torchmetrics' NoTrainInceptionV3 (with torch-fidelity's Inception weights), and torchmetrics "
                                  "cannot be imported here; dmvae_amd does not ship the network.  Pass the feature extractor as a module instead: "
                                  "FID(feature=module), module: uint8 [B, 3, S, S] -> [B, F]") from e
            self.inception = NoTrainInceptionV3(name="inception-v3-compat", features_list=[str(feature)])
            num = int(feature)
        else:
            self.inception = feature
            num = getattr(feature, "num_features", None)
            if num is None:
                p = next(feature.parameters(), None) if isinstance(feature, nn.Module) else None
                probe = torch.zeros(1, 3, self.eval_size, self.eval_size, dtype=torch.uint8, device=p.device if p is not None else "cpu")
                with torch.no_grad():
                    num = feature(probe).shape[-1]
        self.num_features = num = check_feature_width(num, "FID: the feature width")
        for side in _SIDES:
            self.register_buffer(f"{side}_features_sum", torch.zeros(num, dtype=torch.float64))
            self.register_buffer(f"{side}_features_cov_sum", torch.zeros(num, num, dtype=torch.float64))
            self.register_buffer(f"{side}_features_num_samples", torch.tensor(0, dtype=torch.int64))

    # ---- accumulation ------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool) -> None:
        """imgs [B, 3, H, W] in [0, 1] (evaluation/fid.py:57-65): resize to eval_size + quantise, extract, accumulate.  No host synchronisation."""
        if imgs.dtype not in (torch.float32, torch.bfloat16):
            imgs = imgs.float()
        if imgs.is_cuda:
            u8 = ops.fid_resize_u8(imgs.contiguous(), self.eval_size)
        else:
            _stock.require_opt_in("FID.update", "CPU images")
            u8 = _stock_resize_u8(imgs, self.eval_size)
        self.update_features(self.inception(u8), real)

    @torch.no_grad()
    def update_features(self, features: torch.Tensor, real: bool) -> None:
        """features [B, F] (f32, bf16 or f64; anything else is taken as f32) into the real or the fake states, in f64."""
        side = "real" if real else "fake"
        s, c, n = (getattr(self, f"{side}_features_{k}") for k in ("sum", "cov_sum", "num_samples"))
        n += accumulate_features(features, s, c, "FID.update_features")

    # ---- the value ---------------------------------------------------------------------------------
    def _host_states(self):
        """side -> (sum, cov_sum, count) of the six states as `summed_on_host` returns them."""
        host = summed_on_host([getattr(self, f"{side}_features_{k}") for side in _SIDES for k in ("sum", "cov_sum", "num_samples")])
        return {side: (host[3 * i], host[3 * i + 1], int(host[3 * i + 2].item())) for i, side in enumerate(_SIDES)}

    def compute(self) -> torch.Tensor:
        """-> 0-d f64 tensor on the host.  RuntimeError below two samples on either side, as torchmetrics raises."""
        st = self._host_states()
        if st["real"][2] < 2 or st["fake"][2] < 2:
            raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
        mu_r, cov_r = mean_cov(*st["real"])
        mu_f, cov_f = mean_cov(*st["fake"])
        return frechet_distance(mu_r, cov_r, mu_f, cov_f)

    def forward(self, imgs: torch.Tensor, real: bool) -> None:
        self.update(imgs, real)

    def reset(self) -> None:
        for side in _SIDES if self.reset_real_features else ("fake",):
            for k in ("sum", "cov_sum", "num_samples"):
                getattr(self, f"{side}_features_{k}").zero_()

    # ---- statistics in and out ---------------------------------------------------------------------
    def _set(self, side: str, s, c, n) -> None:
        dev, f = self.real_features_sum.device, self.num_features
        s, c = torch.as_tensor(s).to(dev, torch.float64), torch.as_tensor(c).to(dev, torch.float64)
        if tuple(s.shape) != (f,) or tuple(c.shape) != (f, f):
            raise ValueError(f"FID: statistics of width {tuple(s.shape)} / {tuple(c.shape)} do not fit {f} features")
        setattr(self, f"{side}_features_sum", s.contiguous().clone())
        setattr(self, f"{side}_features_cov_sum", c.contiguous().clone())
        setattr(self, f"{side}_features_num_samples", torch.as_tensor(n).to(dev, torch.int64).reshape(()).clone())

    def save(self, real: bool, path) -> None:
        """evaluation/fid.py:67-83: this rank's three states of one side under the reference's keys."""
        side = "real" if real else "fake"
        torch.save({f"{side}_features_{k}": getattr(self, f"{side}_features_{k}") for k in ("sum", "cov_sum", "num_samples")}, path)

    def load(self, real: bool, path) -> None:
        """evaluation/fid.py:85-95."""
        side = "real" if real else "fake"
        d = torch.load(path, map_location="cpu")
        self._set(side, d[f"{side}_features_sum"], d[f"{side}_features_cov_sum"], d[f"{side}_features_num_samples"])

    def statistics(self, real: bool):
        """-> (mu f64 [F], sigma f64 [F, F], n) of this rank's states of one side, on the host (synchronises)."""
        side = "real" if real else "fake"
        n = int(getattr(self, f"{side}_features_num_samples").item())
        if n < 2:
            raise RuntimeError(f"FID.statistics: {n} {side} sample(s); a covariance needs two")
        mu, sigma = mean_cov(getattr(self, f"{side}_features_sum").cpu(), getattr(self, f"{side}_features_cov_sum").cpu(), n)
        return mu, sigma, n

    def load_statistics(self, real: bool, mu, sigma, n: int) -> None:
        """The inverse of `statistics`: precomputed (mu, sigma) of n samples -- tensors or arrays, e.g. the `mu` / `sigma` of a reference-statistics npz --
        become the states sum = n mu, cov_sum = (n - 1) sigma + n mu mu^T."""
        n = int(n)
        if n < 2:
            raise ValueError(f"FID.load_statistics: n must be at least 2, got {n}")
        mu, sigma = torch.as_tensor(mu).to("cpu", torch.float64), torch.as_tensor(sigma).to("cpu", torch.float64)
        self._set("real" if real else "fake", n * mu, (n - 1) * sigma + n * torch.outer(mu, mu), n)
