#!/usr/bin/env python
"""Generates tests/golden/dit_var_*.npz: the reference's own `LightningDiT` (diffusion/lightningdit/lightningdit.py, read from the reference checkout
oracle/capture_golden.py points at) on the CPU in f32, forward and backward, for five configurations of the constructor's block switches away from their
defaults (use_qknorm / use_swiglu / use_rope / use_rmsnorm / wo_shift; the table is tests/dit_variants_spec.py::CFGS).  Same recipe and payload as
oracle/capture_golden_dit.py: deterministic weights regenerated in the tests from names + seed (oracle/detweights.py), x, t, y, out, dy, dx, six full parameter
gradients, norm + sum of every parameter gradient, the fixed position table and the RoPE tables where the configuration has them.  timm (PatchEmbed, Mlp) is
satisfied by capture_golden.install_stubs' stand-ins; its Mlp honours `act_layer` (the tanh-GELU of the non-SwiGLU block).  The fixtures hold tensors, names and
seeds only.

Run:  TORCHDYNAMO_DISABLE=1 python tools/capture_dit_variants_golden.py        (CPU, seconds; the @torch.compile decorators are no-ops then)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import capture_golden as cg  # noqa: E402
from oracle.detweights import det_fill_  # noqa: E402
from dit_variants_spec import CFGS, SEEDS, full_gradient_names  # noqa: E402


def main():
    cg.install_stubs()
    torch.set_grad_enabled(True)
    from diffusion.lightningdit.lightningdit import LightningDiT
    g = torch.Generator().manual_seed(779)               # its own stream: the older fixtures keep theirs
    for tag, kw in CFGS.items():
        m = LightningDiT(**kw).eval()
        fixed = {k: v.clone() for k, v in m.state_dict().items() if k == "pos_embed" or k.startswith("feat_rope")}
        det_fill_(m, SEEDS[tag], skip=("pos_embed",))
        b = 3
        x = torch.randn(b, kw["in_channels"], kw["input_size"], kw["input_size"], generator=g).requires_grad_(True)
        t = torch.rand(b, generator=g)
        y = torch.tensor([1, 10, 4])                      # 10 = the unconditional row of the embedding table
        out = m(x, t, y)
        dy = torch.randn(out.shape, generator=g)
        out.backward(dy)
        grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        cg.save(tag, seed=np.array(SEEDS[tag]), x=x.detach(), t=t, y=y, out=out.detach(), dy=dy, dx=x.grad,
                keys=np.array(list(m.state_dict().keys())), **{"fix." + k: v for k, v in fixed.items()},
                **{"gn." + n: np.array([v.double().norm().item(), v.double().sum().item()]) for n, v in grads.items()},
                **{"g." + n: grads[n] for n in full_gradient_names(kw)})


if __name__ == "__main__":
    main()
