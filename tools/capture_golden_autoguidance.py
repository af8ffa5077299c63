#!/usr/bin/env python
"""Generates tests/golden/autoguidance.npz by running the reference's own `LightningDiT.forward_with_autoguidance` (diffusion/lightningdit/lightningdit.py:450-465,
read from the reference checkout oracle/capture_golden.py points at) on the CPU in f32: two small LightningDiTs with deterministic weights (oracle/detweights.py;
the model of tests/test_oracle_sampler.py with two seeds), the guide's output head perturbed (scaled weight, shifted bias) so that the two outputs differ by
more than their weights' draw, and model times inside, on the edges of and outside the interval, plus the method's default interval.  The fixture holds tensors,
seeds and settings only; tests/test_sampler_methods_host.py rebuilds both models from the seeds.

Run:  TORCHDYNAMO_DISABLE=1 python tools/capture_golden_autoguidance.py        (CPU, seconds)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import capture_golden as cg  # noqa: E402
from oracle.capture_golden_sampler import DIT_KW  # noqa: E402
from oracle.detweights import det_fill_  # noqa: E402

DIT_SEED, GUIDE_SEED = 72, 91
HEAD_SCALE, HEAD_SHIFT = 0.8, 0.05
CFG_SCALE, INTERVAL = 2.5, (0.25, 0.75)
T0 = (0.5, 0.25, 0.75, 0.2, 0.9)          # t[0] of each case: inside, both edges (inclusive), below, above


@torch.no_grad()
def perturb_head_(m):
    m.final_layer.linear.weight.mul_(HEAD_SCALE)
    m.final_layer.linear.bias.add_(HEAD_SHIFT)
    return m


def main():
    cg.install_stubs()
    torch.set_grad_enabled(False)
    from diffusion.lightningdit.lightningdit import LightningDiT
    m = det_fill_(LightningDiT(**DIT_KW).eval(), DIT_SEED, skip=("pos_embed",))
    guide = perturb_head_(det_fill_(LightningDiT(**DIT_KW).eval(), GUIDE_SEED, skip=("pos_embed",)))
    g = torch.Generator().manual_seed(777)
    x = torch.randn(4, 8, 8, 8, generator=g)                # [2n]: the method uses the first half of x, t and y
    y = torch.tensor([3, 10, 7, 0])
    outs = {}
    for i, t0 in enumerate(T0):
        t = torch.tensor([t0, t0, 0.4, 0.6])
        outs[f"t_{i}"] = t
        outs[f"out_{i}"] = m.forward_with_autoguidance(x, t, y, CFG_SCALE, guide.forward, cfg_interval=INTERVAL)
    outs["out_default"] = m.forward_with_autoguidance(x, outs["t_0"], y, CFG_SCALE, guide.forward)       # cfg_interval = (-1e4, -1e4): never inside
    cg.save("autoguidance", x=x, y=y, dit_seed=np.array(DIT_SEED), guide_seed=np.array(GUIDE_SEED), head_scale=np.array(HEAD_SCALE), head_shift=np.array(HEAD_SHIFT),
            cfg_scale=np.array(CFG_SCALE), interval=np.array(INTERVAL), n_cases=np.array(len(T0)), **outs)


if __name__ == "__main__":
    main()
