"""The reference's reconstruction metrics (evaluation/metrics.py) under its own names: `PSNR`, `SSIM`, `LPIPS`.

`SSIM(pred, gt, data_range=1.0)` has the reference's signature and return pair -- (per-image values [T], their mean) for images in [-1, 1] -- without
torchmetrics: the 11 x 11 Gaussian window moments, the SSIM map and its mean are one HIP kernel in f64 (csrc/ssim.hip through `ops.ssim`), deterministic.
torchmetrics runs the same algorithm in the inputs' dtype; in f32 its `E[x^2] - mu^2` loses 3e-5 ... 7e-5 of the per-image value (1e-4 ... 4e-4 with the
newer versions' variance clamp) on near-identical flat images, exactly where a good tokenizer lives (tests/test_ssim_cpu.py prints the figures), so the
two agree to f32's error, not to f64's.  `ssim01` is the same for images already in [0, 1] and returns the f64 values.  bf16 images are widened to f32
first: the value is that of `SSIM(pred.float(), gt.float())`.

CPU tensors take a plain-torch f64 composition behind `DMVAE_ALLOW_STOCK=1`, like every other module (dmvae_amd/_stock.py).

`LPIPS(img1, img2, net_type='alex')` is `dmvae_amd.models.lpips_alex.LPIPSAlex` once a network is configured (`configure_lpips`, DMVAE_LPIPS_ALEX_WEIGHTS,
`run_on_mi355x.py --lpips-weights=PATH`): the weight files are not part of this package, and without one it raises NotImplementedError.  net_type 'vgg'
and 'squeeze' are `dmvae_amd.models.lpips_eval.LPIPSVGG` / `LPIPSSqueeze` in the same way (`configure_lpips(path, net_type=...)`,
DMVAE_LPIPS_VGG_WEIGHTS / DMVAE_LPIPS_SQUEEZE_WEIGHTS, `--lpips-vgg-weights=PATH` / `--lpips-squeeze-weights=PATH`); one network is kept per type."""
from __future__ import annotations

import os
from typing import Tuple

import torch

from . import _stock, ops
from .evaluate import psnr as PSNR

__all__ = ["PSNR", "SSIM", "LPIPS", "ssim01", "configure_lpips", "lpips_network"]

_WIN, _SIGMA, _K1, _K2 = 11, 1.5, 0.01, 0.03


def _stock_ssim01(p: torch.Tensor, t: torch.Tensor, data_range: float) -> torch.Tensor:
    """The CPU route: the valid 11 x 11 filter over the raw images in f64 (what torchmetrics' pad / filter / crop leaves), per-image mean."""
    p, t = p.double(), t.double()
    c = p.shape[1]
    d = torch.arange(_WIN, dtype=torch.float64) - _WIN // 2
    g = torch.exp(-(d / _SIGMA) ** 2 / 2)
    g = g / g.sum()
    kernel = torch.outer(g, g).expand(c, 1, _WIN, _WIN)
    c1, c2 = (_K1 * data_range) ** 2, (_K2 * data_range) ** 2
    mp, mt, epp, ett, ept = (torch.nn.functional.conv2d(x, kernel, groups=c) for x in (p, t, p * p, t * t, p * t))
    sp, st, spt = epp - mp * mp, ett - mt * mt, ept - mp * mt
    m = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (sp + st + c2))
    return m.flatten(1).mean(-1)


def _ssim(a: torch.Tensor, b: torch.Tensor, data_range: float, from_pm1: bool, what: str) -> torch.Tensor:
    if a.dim() != 4 or a.shape != b.shape or a.numel() == 0:
        raise ValueError(f"{what}: expected two non-empty [T, C, H, W] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[-1] < _WIN or a.shape[-2] < _WIN:
        raise ValueError(f"{what}: H and W must be at least {_WIN} (the window has no output below that; torchmetrics returns NaN), got {tuple(a.shape)}")
    data_range = float(data_range)
    if not (data_range > 0 and data_range != float("inf")):
        raise ValueError(f"{what}: data_range must be finite and positive, got {data_range}")
    if a.dtype != b.dtype or a.dtype not in (torch.float32, torch.bfloat16):
        a, b = a.float(), b.float()
    if a.is_cuda:
        return ops.ssim(a.contiguous(), b.contiguous(), data_range=data_range, from_pm1=from_pm1)
    _stock.require_opt_in(what, "CPU images")
    a, b = a.float(), b.float()
    if from_pm1:
        a, b = a.add(1).mul(0.5), b.add(1).mul(0.5)
    return _stock_ssim01(a, b, data_range)


@torch.no_grad()
def ssim01(img1: torch.Tensor, img2: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """[T, C, H, W] images already scaled to [0, 1] -> per-image SSIM, f64 [T]."""
    return _ssim(img1, img2, data_range, False, "metrics.ssim01")


@torch.no_grad()
def SSIM(pred: torch.Tensor, gt: torch.Tensor, data_range: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """evaluation/metrics.py:16-23: [T, C, H, W] images in [-1, 1] -> (per-image SSIM [T], their mean), f32 as the reference returns for f32 inputs; the
    values are computed in f64 and rounded once, the mean is taken over the f64 values."""
    v = _ssim(pred, gt, data_range, True, "metrics.SSIM")
    return v.float(), v.mean().float()


_LPIPS_TYPES = ("alex", "vgg", "squeeze")
_LPIPS_ENV = {"alex": "DMVAE_LPIPS_ALEX_WEIGHTS", "vgg": "DMVAE_LPIPS_VGG_WEIGHTS", "squeeze": "DMVAE_LPIPS_SQUEEZE_WEIGHTS"}
_LPIPS_FLAG = {"alex": "--lpips-weights", "vgg": "--lpips-vgg-weights", "squeeze": "--lpips-squeeze-weights"}
_lpips_net = {t: None for t in _LPIPS_TYPES}                # net_type -> the configured network
_lpips_env_path = {t: None for t in _LPIPS_TYPES}           # net_type -> the file the environment variable's network was built from


def _lpips_class(net_type):
    if net_type == "alex":
        from .models.lpips_alex import LPIPSAlex
        return LPIPSAlex
    from .models import lpips_eval
    return {"vgg": lpips_eval.LPIPSVGG, "squeeze": lpips_eval.LPIPSSqueeze}[net_type]


def _lpips_env(net_type):
    """The file the type's environment variable names, "" when unset."""
    if net_type == "alex":
        return os.environ.get("DMVAE_LPIPS_ALEX_WEIGHTS", "")
    if net_type == "vgg":
        return os.environ.get("DMVAE_LPIPS_VGG_WEIGHTS", "")
    return os.environ.get("DMVAE_LPIPS_SQUEEZE_WEIGHTS", "")


def _lpips_type(net_type):
    if net_type not in _LPIPS_TYPES:
        raise ValueError(f"metrics.LPIPS: net_type must be 'alex', 'vgg' or 'squeeze', got {net_type!r}")
    return net_type


def configure_lpips(net_or_path, net_type=None):
    """Gives `LPIPS` its network of one type: a `dmvae_amd.models.lpips_alex.LPIPSAlex`, `dmvae_amd.models.lpips_eval.LPIPSVGG` or `LPIPSSqueeze` (the
    module selects its type), the path of one state_dict file (`from_checkpoint` of net_type's class, default 'alex'), a (trunk_path, lin_path) pair
    (`from_checkpoints`), or None to unconfigure net_type -- all three types when no net_type is given.  One network is kept per type.  Returns the
    network.  The weight files are not part of this package."""
    if net_or_path is None:
        for t in _LPIPS_TYPES if net_type is None else (_lpips_type(net_type),):
            _lpips_net[t], _lpips_env_path[t] = None, None
        return None
    own = [t for t in _LPIPS_TYPES if isinstance(net_or_path, _lpips_class(t))]
    if own:
        if net_type is not None and net_type != own[0]:
            raise ValueError(f"metrics.configure_lpips: a {type(net_or_path).__name__} is net_type {own[0]!r}, not {net_type!r}")
        kind, net = own[0], net_or_path
    else:
        kind = _lpips_type("alex" if net_type is None else net_type)
        cls = _lpips_class(kind)
        net = cls.from_checkpoints(*net_or_path) if isinstance(net_or_path, (tuple, list)) else cls.from_checkpoint(net_or_path)
    _lpips_net[kind], _lpips_env_path[kind] = net, None
    return net


def lpips_network(net_type="alex"):
    """The network `LPIPS` runs for net_type: the one `configure_lpips` was given, else one built (once) from the file DMVAE_LPIPS_ALEX_WEIGHTS /
    DMVAE_LPIPS_VGG_WEIGHTS / DMVAE_LPIPS_SQUEEZE_WEIGHTS names, else None."""
    kind = _lpips_type(net_type)
    if _lpips_net[kind] is not None and _lpips_env_path[kind] is None:
        return _lpips_net[kind]                                      # configured explicitly
    path = _lpips_env(kind)
    if path != (_lpips_env_path[kind] or ""):                        # the variable appeared, moved or went away: so does what it configured
        configure_lpips(path or None, kind)
        _lpips_env_path[kind] = path or None
    return _lpips_net[kind]


@torch.no_grad()
def LPIPS(img1, img2, net_type="alex"):
    """evaluation/metrics.py:26-29: [T, 3, H, W] images in [-1, 1] -> torchmetrics' LearnedPerceptualImagePatchSimilarity(net_type, reduction='mean'), an f32
    scalar on the inputs' device: the mean over the images of the configured network's `forward` (dmvae_amd/models/lpips_alex.py, lpips_eval.py: the
    library's published definition restated -- the library cannot be run where this package is developed -- on the exact-f32 convolution kernels and an f64
    head; the mean is taken over the f64 values and rounded once).  The backbones and the linear heads are weights this package does not hold: name them
    with `configure_lpips(path, net_type)`, DMVAE_LPIPS_{ALEX,VGG,SQUEEZE}_WEIGHTS or `run_on_mi355x.py --lpips-weights=PATH` /
    `--lpips-vgg-weights=PATH` / `--lpips-squeeze-weights=PATH`.  `dmvae_amd.losses` / utils/lpips.py is the TRAINING loss: VGG16 in bf16 with the
    reference's own normalisation (`LPIPSVGG(normalize="reference")` is its exact-f32 twin), not torchmetrics' 'vgg' numbers."""
    kind = _lpips_type(net_type)
    net = lpips_network(kind)
    if net is None and kind != "alex":
        raise NotImplementedError(f"metrics.LPIPS: net_type {kind!r} is not built in this process: no weights configured (configure_lpips(path, "
                                  f"net_type={kind!r}), {_LPIPS_ENV[kind]}, {_LPIPS_FLAG[kind]}=PATH)")
    if net is None:
        raise NotImplementedError("metrics.LPIPS has no network: the reference's evaluation LPIPS is torchmetrics' AlexNet network, whose weights are not part of "
                                  "this package or of the reference repo (configure_lpips(path), DMVAE_LPIPS_ALEX_WEIGHTS or --lpips-weights=PATH names "
                                  "them), and utils/lpips.py is the training loss's VGG16 -- not a substitute for it")
    if torch.is_tensor(img1) and next(net.parameters()).device != img1.device:
        net.to(img1.device)
    return net(img1, img2).mean().float()
