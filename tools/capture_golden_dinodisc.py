#!/usr/bin/env python
"""Captures tests/golden/dinodisc_{small,branches,manifest}.npz from the reference's own models/dinodisc.py + models/dinov2.py on the CPU (f32).

    python tools/capture_golden_dinodisc.py            (DMVAE_REFERENCE: the reference checkout)

Imports go through oracle.capture_golden.install_stubs() plus two more stand-ins that carry no arithmetic of the model: `utils.dist` (only reached by the
SyncBatchNorm head variants) and torchvision's `RandomCrop`, written here as what its documentation says -- offsets from `torch.randint(0, h - th + 1, (1,))`
then `torch.randint(0, w - tw + 1, (1,))`, then the crop (torchvision is not a dependency: unpinned).  A 4-block ViT-S is registered under its own
`dino_size` name; its checkpoint and the heads are filled by name (tests/dinodisc_spec.py: filled_backbone / filled_heads), so the tests rebuild the same
weights from the seeds and only results are stored."""
import importlib
import os
import random
import sys
import tempfile
import types
from functools import partial

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import capture_golden as CG  # noqa: E402
import dinodisc_spec as S  # noqa: E402


class RandomCrop:
    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        h, w = img.shape[-2:]
        th, tw = self.size
        i = int(torch.randint(0, h - th + 1, size=(1,)).item())
        j = int(torch.randint(0, w - tw + 1, size=(1,)).item())
        return img[..., i:i + th, j:j + tw]


def reference_modules():
    CG.install_stubs()
    if "utils" not in sys.modules or not hasattr(sys.modules["utils"], "__path__"):
        pkg = types.ModuleType("utils")
        pkg.__path__ = [os.path.join(CG.REF, "utils")]
        sys.modules["utils"] = pkg
    dist = types.ModuleType("utils.dist")
    dist.new_local_machine_group = lambda: None
    sys.modules["utils.dist"] = dist
    sys.modules["utils"].dist = dist
    sys.modules["torchvision.transforms"].RandomCrop = RandomCrop
    dinov2 = importlib.import_module("models.dinov2")
    dinodisc = importlib.import_module("models.dinodisc")
    dinov2.__dict__["vit_small_d4"] = lambda **kw: dinov2.DinoVisionTransformer(
        embed_dim=384, depth=4, num_heads=6, mlp_ratio=4, block_fn=partial(dinov2.Block, attn_class=dinov2.MemEffAttention), **kw)
    return dinov2, dinodisc


def build(dinodisc, arch, seed, **kw):
    vit = dinodisc.make_dinov2_model(arch_name=arch)
    sd = S.filled_backbone({k: v.shape for k, v in vit.state_dict().items()}, seed)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "dino.pth")
        torch.save(sd, path)
        disc = dinodisc.DinoDisc(device="cpu", dino_ckpt=path, dino_size=arch, **kw)
    heads = S.filled_heads({k: v.shape for k, v in disc.state_dict().items()}, seed)
    disc.load_state_dict(heads, strict=False)
    return disc, vit, heads


def grads_record(out, named):
    for k, g in named:
        g = g.detach()
        if g.numel() < 4096:
            out["g." + k] = g.numpy()
        else:
            stride = 97 if g.numel() < 200000 else 997
            out["gs." + k] = g.flatten()[::stride].numpy()
            out["gn." + k] = np.float64(g.double().norm().item())
            out["gsum." + k] = np.float64(g.double().sum().item())


def main():
    dinov2, dinodisc = reference_modules()
    c = S.SMALL
    # ---- dinodisc_small: train-mode logits + head gradients, eval-mode logits + input gradient --------------------------------------------------------------
    random_random = random.random
    random.random = lambda: 0.75                                   # > 0.5: the area branch
    try:
        disc, _, heads = build(dinodisc, "vit_small_d4", c["seed"], ks=c["ks"], key_depths=c["key_depths"])
        x = S.image(c["batch"], c["px"], c["x_seed"])
        disc.train()
        logits = disc(x)
        dy = torch.randn(logits.shape, generator=torch.Generator().manual_seed(c["dy_seed"]))
        (logits * dy).sum().backward()
        out = {"logits_train": logits.detach().numpy()}
        for k, v in disc.state_dict().items():
            if k.endswith("weight_u") or k.endswith("weight_v"):
                out["uv." + k] = v.numpy().copy()
        grads_record(out, [(k, p.grad) for k, p in disc.named_parameters()])
        disc.load_state_dict(heads, strict=False)                  # the buffers as before the train call
        disc.eval().requires_grad_(False)
        xe = x.clone().requires_grad_(True)
        le = disc(xe)
        (le * dy).sum().backward()
        out.update(logits_eval=le.detach().numpy(), dx_slice=xe.grad[:, :, ::16, ::16].numpy().copy(), dx_norm=np.float64(xe.grad.double().norm().item()))
    finally:
        random.random = random_random
    np.savez_compressed(os.path.join(CG.OUT, "dinodisc_small.npz"), **out)
    # ---- dinodisc_branches: B = 2, forward only -------------------------------------------------------------------------------------------------------------
    out = {}
    with torch.no_grad():
        rs = next(s for s in range(100) if random.Random(s).random() <= 0.5)
        random.seed(rs)
        torch.manual_seed(11)
        out.update(crop_random_seed=np.int64(rs), crop_torch_seed=np.int64(11), crop=disc(S.image(2, 256, 7)).numpy())
        out["px252"] = disc(S.image(2, 252, 8)).numpy()
        out["px70"] = disc(S.image(2, 70, 9)).numpy()
    np.savez_compressed(os.path.join(CG.OUT, "dinodisc_branches.npz"), **out)
    # ---- dinodisc_manifest: the default full-size module's state_dict and the checkpoint format ---------------------------------------------------------------
    full, vit, _ = build(dinodisc, "vit_small", 1, ks=9)

    def table(sd):
        keys = list(sd.keys())
        shapes = np.full((len(keys), 4), -1, dtype=np.int64)
        for i, k in enumerate(keys):
            shapes[i, :sd[k].dim()] = list(sd[k].shape)
        return np.array(keys), shapes
    dk, ds = table(full.state_dict())
    ck, cs = table(vit.state_dict())
    np.savez_compressed(os.path.join(CG.OUT, "dinodisc_manifest.npz"), disc_keys=dk, disc_shapes=ds, ckpt_keys=ck, ckpt_shapes=cs)
    for n in ("small", "branches", "manifest"):
        print(n, os.path.getsize(os.path.join(CG.OUT, f"dinodisc_{n}.npz")), "bytes")


if __name__ == "__main__":
    main()
