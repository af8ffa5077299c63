#!/usr/bin/env python
"""Run one of the reference's scripts on the MI355X kernels without editing it.

    python run_on_mi355x.py /path/to/dmvae/train_tokenizer.py --local_bs 32 ...
    torchrun --nproc-per-node 8 run_on_mi355x.py /path/to/dmvae/train_dmd.py ...
    python run_on_mi355x.py --check            # print what is shadowed and exit
    python run_on_mi355x.py --hip-dinodisc /path/to/dmvae/train_tokenizer.py --disc_type dino ...      (or DMVAE_HIP_DINODISC=1)
    python run_on_mi355x.py --hip-optim /path/to/dmvae/train_tokenizer.py ...                          (or DMVAE_HIP_OPTIM=1)
    python run_on_mi355x.py --hip-fid /path/to/dmvae/train_tokenizer.py ...                            (or DMVAE_HIP_FID=1)
    python run_on_mi355x.py --hip-metrics /path/to/dmvae/script.py ...                                 (or DMVAE_HIP_METRICS=1)
    python run_on_mi355x.py --lpips-weights=/path/to/lpips_alex.pth /path/to/dmvae/script.py ...       (implies --hip-metrics)
    python run_on_mi355x.py --lpips-vgg-weights=PATH --lpips-squeeze-weights=PATH /path/to/dmvae/script.py ...   (net_type 'vgg' / 'squeeze'; imply --hip-metrics)

The reference's drivers import their model code by module path (`from models.vae import VAE`, `from utils.lpips import LPIPS`,
`from diffusion.lightningdit.lightningdit import LightningDiT_models`, `from diffusion.transport import create_transport`; train_tokenizer.py:10-17,
train_dmd.py:10-17, train_diffusion.py:15-17, sample_50k.py:6-14).  `install_shadow()` registers this build's mirrors under exactly those module paths --
same class names, constructor arguments, forward signatures and state_dict keys, HIP kernels underneath -- before the script runs.  Everything else the
scripts import (utils.dist, utils.build_dataset, evaluation.*, models.dinodisc, models.init_param's callers ...) still resolves to the reference's own
files: the shadow packages keep the reference's directories on their __path__.

`models.dinodisc` / `models.DinoDisc` (--disc_type dino) is an opt-in: by default it stays the reference's file; `--hip-dinodisc` in front of the script path,
DMVAE_HIP_DINODISC=1 or `install_shadow(ref, dinodisc=True)` registers this build's `dmvae_amd.models.dinodisc` instead and turns its SyncBatchNorm head
variants on (`enable_syncbn_heads`): the scripts' default is `--disc_norm sbn`.

The optimiser tail is an opt-in too: `--hip-optim` in front of the script path (in either order with `--hip-dinodisc`), DMVAE_HIP_OPTIM=1 or
`install_shadow(ref, optim=True)` makes `torch.optim.AdamW` and `torch.nn.utils.clip_grad_norm_` this build's `dmvae_amd.optim.AdamW` / `clip_grad_norm_` for the
process (train_tokenizer.py:382-383,415,424): multi-tensor HIP kernels over the scripts' own parameters.  Without it nothing in `torch` is touched.  The scripts'
`update_ema` is defined in the scripts themselves and cannot be replaced from outside; `from dmvae_amd.optim import update_ema` is the one-line edit.

`evaluation.fid` (`from evaluation.fid import FID`, train_tokenizer.py:20, train_dmd.py:20) is an opt-in as well: `--hip-fid` in front of the script path (in any
order with the other two), DMVAE_HIP_FID=1 or `install_shadow(ref, fid=True)` registers `dmvae_amd.fid` under that path: the resize and the f64 feature
statistics on this build's kernels.  `FID()` as the scripts call it (feature=2048) still needs torchmetrics for the Inception network itself -- unless an
Inception weight file is named: `--inception-weights=/path/to/pt_inception-2015-12-05.pth` (implies --hip-fid) or `install_shadow(ref, fid=True,
inception_weights=path)` registers `dmvae_amd.models.inception.fid_module(path)` instead, `dmvae_amd.fid`'s names with an `FID` whose int `feature` (2048
only) builds this build's `InceptionV3Compat` from that file: the network on the exact-f32 kernels, no torchmetrics.

`evaluation.metrics` (`PSNR`, `SSIM`, `LPIPS`) is an opt-in too: `--hip-metrics`, DMVAE_HIP_METRICS=1 or `install_shadow(ref, metrics=True)` registers
`dmvae_amd.metrics` under that path: `SSIM` on this build's f64 kernel with no torchmetrics import, `PSNR` unchanged, `LPIPS` a NotImplementedError (its AlexNet
weights are not here) -- unless a weight file is named: `--lpips-weights=/path/to/state_dict.pth` (implies --hip-metrics), DMVAE_LPIPS_ALEX_WEIGHTS or
`install_shadow(ref, metrics=True, lpips_weights=path)` hands it to `dmvae_amd.metrics.configure_lpips`, and `LPIPS` is then this build's
`dmvae_amd.models.lpips_alex.LPIPSAlex` for net_type 'alex'; `--lpips-vgg-weights=PATH` and `--lpips-squeeze-weights=PATH` (or DMVAE_LPIPS_VGG_WEIGHTS /
DMVAE_LPIPS_SQUEEZE_WEIGHTS) name the files of `dmvae_amd.models.lpips_eval.LPIPSVGG` / `LPIPSSqueeze` for net_type 'vgg' / 'squeeze'.  Without the opt-in the reference's file keeps serving it.

The GVP / VP paths of `diffusion.transport` are off in the mirror by default (`dmvae_amd.transport.enable_all_paths`).  Running a script turns them on -- the
script's own `--path_type` is the selection --; `--check` and a bare `install_shadow(ref)` leave the switch alone (`install_shadow(ref, all_paths=True)` asks)."""
from __future__ import annotations

import importlib
import os
import runpy
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# module path the reference imports -> this build's module
SHADOWS = {
    "models.vae": "dmvae_amd.models.vae",                                  # VAE, DINOEncoder, MLP            (models/vae.py)
    "models.flux_ae": "dmvae_amd.models.flux_ae",                          # Decoder, Encoder, ResnetBlock...  (models/flux_ae.py)
    "models.init_param": "dmvae_amd.models.init_param",                    # init_weights                      (models/init_param.py)
    "models.patchgan": "dmvae_amd.models.patchgan",                        # NLayerDiscriminator               (models/patchgan.py)
    "utils.lpips": "dmvae_amd.utils.lpips",                                # LPIPS                             (utils/lpips.py)
    "utils.diffaug": "dmvae_amd.utils.diffaug",                            # DiffAug                           (utils/diffaug.py)
    "diffusion.lightningdit.lightningdit": "dmvae_amd.models.lightningdit",   # LightningDiT, LightningDiT_models (diffusion/lightningdit/lightningdit.py)
    "diffusion.transport": "dmvae_amd.transport",                          # create_transport, Transport, Sampler (diffusion/transport/__init__.py)
}


def _package(name: str, ref_dir: str | None) -> types.ModuleType:
    """A namespace-like package module whose __path__ is the reference's directory of that name (so that sub-modules this build does not shadow still
    import from the reference), registered in sys.modules."""
    mod = sys.modules.get(name)
    if mod is None or not hasattr(mod, "__path__"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    if ref_dir:
        d = os.path.join(ref_dir, *name.split("."))
        if os.path.isdir(d) and d not in mod.__path__:
            mod.__path__.append(d)
    return mod


def install_optim() -> dict:
    """Replace torch.optim.AdamW and torch.nn.utils.clip_grad_norm_ for this process (dmvae_amd.optim.install); returns {attribute path: object}."""
    return importlib.import_module("dmvae_amd.optim").install()


def install_shadow(ref_dir: str | None = None, dinodisc: bool = False, optim: bool = False, all_paths: bool = False, fid: bool = False,
                   metrics: bool = False, inception_weights: str | None = None, lpips_weights: str | None = None) -> dict:
    """Register the mirrors; returns {shadowed module path: module}.  `ref_dir`: root of the reference checkout (None: only the shadowed modules resolve).
    dinodisc: also shadow models.dinodisc / models.DinoDisc with this build's (default: the reference's own file serves them).
    optim: also replace torch.optim.AdamW and torch.nn.utils.clip_grad_norm_ (`install_optim`; not part of the returned dict).
    all_paths: also let the transport mirror build the GVP / VP plans (`dmvae_amd.transport.enable_all_paths`; default: left as it is).
    fid: also shadow evaluation.fid with this build's `dmvae_amd.fid` (default: the reference's own file serves it).
    metrics: also shadow evaluation.metrics with this build's `dmvae_amd.metrics` (default: the reference's own file serves it).
    inception_weights (with fid): a state_dict file of torch-fidelity's Inception network; evaluation.fid becomes
    `dmvae_amd.models.inception.fid_module(path)`, whose `FID(feature=2048)` runs this build's network instead of asking torchmetrics for one.
    lpips_weights (with metrics): a state_dict file of the evaluation LPIPS' AlexNet trunk and lin heads (`LPIPSAlex.from_checkpoint`); it is loaded here and
    handed to `dmvae_amd.metrics.configure_lpips`, so that evaluation.metrics.LPIPS computes instead of raising."""
    if inception_weights and not fid:
        raise ValueError("install_shadow: inception_weights needs fid=True")
    if lpips_weights and not metrics:
        raise ValueError("install_shadow: lpips_weights needs metrics=True")
    out = {}
    shadows = dict(SHADOWS)
    if dinodisc:
        shadows["models.dinodisc"] = "dmvae_amd.models.dinodisc"           # DinoDisc                          (models/dinodisc.py)
    if fid:
        shadows["evaluation.fid"] = "dmvae_amd.fid"                        # FID                               (evaluation/fid.py)
    if metrics:
        shadows["evaluation.metrics"] = "dmvae_amd.metrics"                # PSNR, SSIM, LPIPS                 (evaluation/metrics.py)
    for path, target in shadows.items():
        parts = path.split(".")
        for i in range(1, len(parts)):
            _package(".".join(parts[:i]), ref_dir)
        mod = importlib.import_module(target)
        if path == "evaluation.fid" and inception_weights:
            mod = importlib.import_module("dmvae_amd.models.inception").fid_module(inception_weights)
        if path == "evaluation.metrics" and lpips_weights:
            mod.configure_lpips(lpips_weights)
        sys.modules[path] = mod
        setattr(sys.modules[".".join(parts[:-1])], parts[-1], mod)
        out[path] = mod
    models = sys.modules["models"]
    # models/__init__.py re-exports three names (train_dmd.py:10: `from models import VAE, DinoDisc, NLayerDiscriminator`)
    models.VAE = out["models.vae"].VAE
    models.NLayerDiscriminator = out["models.patchgan"].NLayerDiscriminator

    if dinodisc:
        models.DinoDisc = out["models.dinodisc"].DinoDisc
        out["models.dinodisc"].enable_syncbn_heads()                       # the scripts pass norm_type "sbn" (train_tokenizer.py:48-49, train_dmd.py:50-51)

    def _lazy(name):          # DinoDisc stays the reference's own unless opted in: imported from its file on first use
        if name == "DinoDisc":
            return importlib.import_module("models.dinodisc").DinoDisc
        raise AttributeError(f"module 'models' has no attribute {name!r}")
    models.__getattr__ = _lazy
    if optim:
        install_optim()
    if all_paths:
        out["diffusion.transport"].enable_all_paths()
    return out


def main(argv) -> int:
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    hip_dinodisc = os.environ.get("DMVAE_HIP_DINODISC", "0") not in ("", "0")
    hip_optim = importlib.import_module("dmvae_amd.optim").requested()      # DMVAE_HIP_OPTIM=1
    hip_fid = os.environ.get("DMVAE_HIP_FID", "0") not in ("", "0")
    hip_metrics = os.environ.get("DMVAE_HIP_METRICS", "0") not in ("", "0")
    weights = lpips_weights = None
    lpips_more = {}                                  # net_type -> file, for the evaluation LPIPS' 'vgg' and 'squeeze' networks
    while argv and (argv[0] in ("--hip-dinodisc", "--hip-optim", "--hip-fid", "--hip-metrics") or
                    argv[0].startswith(("--inception-weights=", "--lpips-weights=", "--lpips-vgg-weights=", "--lpips-squeeze-weights="))):
        if argv[0].startswith("--inception-weights="):
            weights, hip_fid = argv[0].split("=", 1)[1], True
        elif argv[0].startswith(("--lpips-vgg-weights=", "--lpips-squeeze-weights=")):
            lpips_more[argv[0].split("-")[3]], hip_metrics = argv[0].split("=", 1)[1], True
        elif argv[0].startswith("--lpips-weights="):
            lpips_weights, hip_metrics = argv[0].split("=", 1)[1], True
        elif argv[0] == "--hip-dinodisc":
            hip_dinodisc = True
        elif argv[0] == "--hip-fid":
            hip_fid = True
        elif argv[0] == "--hip-metrics":
            hip_metrics = True
        else:
            hip_optim = True
        argv = argv[1:]
    if not argv:
        print(__doc__)
        return 0
    def more_lpips(shadowed):                        # after install_shadow: the shadowed evaluation.metrics is dmvae_amd.metrics
        for net_type, path in lpips_more.items():
            net = shadowed["evaluation.metrics"].configure_lpips(path, net_type=net_type)
            print(f"evaluation.metrics.LPIPS(net_type={net_type!r}) -> {type(net).__module__}.{type(net).__name__} ({path})")
    if argv[0] == "--check":
        ref = argv[1] if len(argv) > 1 else None
        shadowed = install_shadow(ref, dinodisc=hip_dinodisc, fid=hip_fid, metrics=hip_metrics, inception_weights=weights, lpips_weights=lpips_weights)
        for path, mod in shadowed.items():
            print(f"{path:40s} -> {mod.__name__}")
        more_lpips(shadowed)
        if hip_optim:
            for path, obj in install_optim().items():
                print(f"{path:40s} -> {obj.__module__}.{obj.__qualname__}")
        return 0
    script = os.path.abspath(argv[0])
    ref = os.path.dirname(script)
    more_lpips(install_shadow(ref, dinodisc=hip_dinodisc, optim=hip_optim, all_paths=True, fid=hip_fid, metrics=hip_metrics, inception_weights=weights,
                              lpips_weights=lpips_weights))      # the script's --path_type selects
    if ref not in sys.path:
        sys.path.insert(0, ref)                     # what `python script.py` would have put first
    sys.argv = [script] + list(argv[1:])
    runpy.run_path(script, run_name="__main__")
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
