#!/usr/bin/env python
"""Captures tests/golden/dinodisc_sbn_{small,manifest}.npz from the reference's own models/dinodisc.py + models/dinov2.py on the CPU (f32, one process), in the
configuration its trainers build: norm_type "sbn" (nn.SyncBatchNorm), use_specnorm False, norm_eps 1e-6 (train_tokenizer.py:48-49,307-314).

    python tools/capture_golden_dinodisc_sbn.py            (DMVAE_REFERENCE: the reference checkout)
    python tools/capture_golden_dinodisc_sbn.py --pick-seed      how SMALL["seed"] of tests/dinodisc_sbn_spec.py was chosen (see pick_seed)

The reference is imported at run time through tools/capture_golden_dinodisc.py's `reference_modules()` / `build()` and its stand-ins; parameters and buffers are
filled by name (tests/dinodisc_sbn_spec.py: filled_heads -- running_var positive, num_batches_tracked an integer), so only results are stored:
  small     4-block ViT-S, ks 9, key_depths (0, 3), 256 px (the area branch), B = 12: train-mode logits of two consecutive calls (two images), the running
            statistics and num_batches_tracked after each, the parameter gradients of the first call; eval-mode logits and input-gradient slices with the filled
            (not the initial 0 / 1) running statistics
  manifest  state_dict keys and shapes of the full-size module with key_depths (0, 2, 5, 8, 11)"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import capture_golden_dinodisc as CD  # noqa: E402
import dinodisc_spec as S  # noqa: E402
import dinodisc_sbn_spec as SB  # noqa: E402
from oracle import capture_golden as CG  # noqa: E402

STATE = ("running_mean", "running_var", "num_batches_tracked")
SEEDS = range(37, 61)


def kink_margin(dinodisc, seed):
    """The smallest |pre-activation| (a SyncBatchNorm's output, LeakyReLU's input) in the reference's f32 train- and eval-mode runs on the captured image."""
    c = SB.SMALL
    disc, _, _ = CD.build(dinodisc, "vit_small_d4", seed, ks=c["ks"], key_depths=c["key_depths"], norm_type="sbn", norm_eps=c["norm_eps"], use_specnorm=False)
    heads = SB.filled_heads({k: v.shape for k, v in disc.state_dict().items()}, seed)
    disc.load_state_dict(heads, strict=False)
    seen = []
    hooks = [m.register_forward_hook(lambda mod, i, o: seen.append(o.abs().min().item())) for m in disc.modules() if isinstance(m, torch.nn.SyncBatchNorm)]
    x = S.image(c["batch"], c["px"], c["x_seed"])
    with torch.no_grad():
        disc.train()
        disc(x)
        disc.load_state_dict(heads, strict=False)
        disc.eval()
        disc(x)
    for h in hooks:
        h.remove()
    assert len(seen) == 4 * len(c["key_depths"])
    return min(seen)


def pick_seed(dinodisc):
    """LeakyReLU's derivative jumps at zero: a pre-activation within f32 rounding noise of it (1e-7 ... 1e-6 at these magnitudes) is on either side depending on
    the order of an f32 sum, and one such element moves single gradient entries by 1e-4 ... 5e-3 of the tensor's largest -- past the 1e-4 bars, in any two correct
    f32 statements of the module.  Among 6 M pre-activations some always come close; the fixture's seed is the one of SEEDS whose closest one is farthest."""
    margins = {s: kink_margin(dinodisc, s) for s in SEEDS}
    for s, m in margins.items():
        print(f"seed {s}: smallest |pre-activation| {m:.3e}")
    return max(margins, key=margins.get)


def main():
    _, dinodisc = CD.reference_modules()
    c = SB.SMALL
    random.random = lambda: 0.75
    if "--pick-seed" in sys.argv:
        print("seed with the widest margin:", pick_seed(dinodisc), "(tests/dinodisc_sbn_spec.py SMALL['seed'])")
        return
    kw = dict(norm_type="sbn", norm_eps=c["norm_eps"], use_specnorm=False)
    random_random = random.random
    random.random = lambda: 0.75                                   # > 0.5: the area branch
    try:
        disc, _, _ = CD.build(dinodisc, "vit_small_d4", c["seed"], ks=c["ks"], key_depths=c["key_depths"], **kw)
        heads = SB.filled_heads({k: v.shape for k, v in disc.state_dict().items()}, c["seed"])
        disc.load_state_dict(heads, strict=False)
        x, x2 = S.image(c["batch"], c["px"], c["x_seed"]), S.image(c["batch"], c["px"], c["x_seed"] + 1)
        disc.train()
        logits = disc(x)
        dy = torch.randn(logits.shape, generator=torch.Generator().manual_seed(c["dy_seed"]))
        (logits * dy).sum().backward()
        out = {"logits_train": logits.detach().numpy()}
        out.update({"st1." + k: v.numpy().copy() for k, v in disc.state_dict().items() if k.endswith(STATE)})
        CD.grads_record(out, [(k, p.grad) for k, p in disc.named_parameters()])
        with torch.no_grad():
            out["logits_train2"] = disc(x2).numpy()
        out.update({"st2." + k: v.numpy().copy() for k, v in disc.state_dict().items() if k.endswith(STATE)})
        disc.load_state_dict(heads, strict=False)                  # the buffers as before the train calls
        disc.eval().requires_grad_(False)
        xe = x.clone().requires_grad_(True)
        le = disc(xe)
        (le * dy).sum().backward()
        out.update(logits_eval=le.detach().numpy(), dx_slice=xe.grad[:, :, ::16, ::16].numpy().copy(), dx_norm=np.float64(xe.grad.double().norm().item()))
        assert all(torch.equal(v, heads[k]) for k, v in disc.state_dict().items() if k.endswith(STATE))      # eval: the estimates are constants
    finally:
        random.random = random_random
    np.savez_compressed(os.path.join(CG.OUT, "dinodisc_sbn_small.npz"), **out)
    full, _, _ = CD.build(dinodisc, "vit_small", 1, ks=9, key_depths=(0, 2, 5, 8, 11), **kw)
    sd = full.state_dict()
    keys = list(sd.keys())
    shapes = np.full((len(keys), 4), -1, dtype=np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    np.savez_compressed(os.path.join(CG.OUT, "dinodisc_sbn_manifest.npz"), disc_keys=np.array(keys), disc_shapes=shapes)
    for n in ("small", "manifest"):
        print(n, os.path.getsize(os.path.join(CG.OUT, f"dinodisc_sbn_{n}.npz")), "bytes")
    print(len(disc.state_dict()), "state_dict keys,", sum(1 for _ in disc.parameters()), "parameters")


if __name__ == "__main__":
    main()
