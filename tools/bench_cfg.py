#!/usr/bin/env python
"""Guided sampling, three routes in one process: LightningDiT-XL/1 at sample_50k's batch (n = 25 latents of 32 x 16 x 16, so the guided state is 2n = 50),
Euler-Maruyama SDE sampler, `forward_with_cfg` with cfg_scale 4 on all channels, under autocast(bf16):

  (a) the tensor-op composition over the ungraphed forward (`LightningDiT.forward_with_cfg_composed`: what forward_with_cfg was before the guidance kernel),
  (b) the kernel route ungraphed (`forward_with_cfg`: 2n forward + ops.cfg_combine),
  (c) the kernel route as one hipGraph replay per evaluation (`lightningdit_fast.GraphedInferenceCfg`),

and with the cfg_interval gate on, (a) -- one host synchronisation per evaluation for the test of t[0] -- against (c), whose gate is compared on the device.
The routes alternate within every round after one untimed round; each run is timed with device events around the whole sampler call.  Prints one JSON line:
milliseconds per sampler step (median over the rounds, and every round), the spread of (a) ((max - min) / median over its rounds), the ratios (b)/(a), (c)/(a)
and gate (c)/(a), the device clock during the timed region, and whether the three routes' last states are bit-identical.  Random DiT weights: the time per step
does not depend on them.

  python tools/bench_cfg.py [--steps 250] [--rounds 4] [--n 25] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from bench import GpuEnvSampler
from dmvae_amd.models import lightningdit_fast as fast
from dmvae_amd.models.lightningdit import LightningDiT_models
from dmvae_amd.sample import cfg_inputs
from dmvae_amd.transport import Sampler, create_transport

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=250)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--n", type=int, default=25)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_cfg.py measures on the GPU"

BF, SCALE, START = torch.bfloat16, 4.0, 0.5
torch.manual_seed(0)
dit = LightningDiT_models["LightningDiT-XL/1"](input_size=16, in_channels=32, num_classes=1000).cuda().eval().requires_grad_(False)
with torch.no_grad():
    for blk in dit.blocks:
        blk.adaLN_modulation[1].weight.normal_(0, 0.02)
    dit.final_layer.linear.weight.normal_(0, 0.02)
z = torch.randn(args.n, 32, 16, 16, device="cuda")
y = torch.randint(0, 1000, (args.n,), device="cuda")
zz, yy = cfg_inputs(z, y, 1000)
sample_fn = Sampler(create_transport()).sample_sde(sampling_method="Euler", diffusion_form="sigma", last_step="Mean", last_step_size=0.04, num_steps=args.steps)
kw = dict(cfg_scale=SCALE, standard_cfg=True)
kw_gate = dict(kw, cfg_interval=True, cfg_interval_start=START)


def run(model_fn, more):
    torch.manual_seed(1)                                             # the same noise stream for every route
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        torch.cuda.synchronize()
        a.record()
        last = sample_fn(zz, model_fn, y=yy, **more)[-1]
        b.record()
        b.synchronize()
    return a.elapsed_time(b) / args.steps, last.clone()


with torch.no_grad(), torch.autocast("cuda", dtype=BF):
    t0 = torch.zeros(2 * args.n, device="cuda")
    graphed = fast.GraphedInferenceCfg(dit, zz, t0, yy, **kw)
    graphed_gate = fast.GraphedInferenceCfg(dit, zz, t0, yy, **kw_gate)
routes = [("a_composed", dit.forward_with_cfg_composed, kw), ("b_kernel", dit.forward_with_cfg, kw), ("c_kernel_graphed", graphed, kw),
          ("gate_a_composed", dit.forward_with_cfg_composed, kw_gate), ("gate_c_kernel_graphed", graphed_gate, kw_gate)]
times, last = {name: [] for name, *_ in routes}, {}
for name, fn, more in routes:                                        # the untimed round: every shape, every route
    run(fn, more)
env = GpuEnvSampler(0)
env.start()
for _ in range(args.rounds):
    for name, fn, more in routes:
        ms, last[name] = run(fn, more)
        times[name].append(ms)
clock = env.stop()
med = {k: statistics.median(v) for k, v in times.items()}
a = times["a_composed"]
line = {"bench": "cfg_sampler", "model": "LightningDiT-XL/1", "n": args.n, "state": 2 * args.n, "steps": args.steps, "rounds": args.rounds, "cfg_scale": SCALE,
        "ms_per_step": {k: round(v, 4) for k, v in med.items()}, "ms_per_step_rounds": {k: [round(x, 4) for x in v] for k, v in times.items()},
        "spread_a": round((max(a) - min(a)) / med["a_composed"], 5),
        "ratio_b_over_a": round(med["b_kernel"] / med["a_composed"], 5), "ratio_c_over_a": round(med["c_kernel_graphed"] / med["a_composed"], 5),
        "ratio_gate_c_over_gate_a": round(med["gate_c_kernel_graphed"] / med["gate_a_composed"], 5),
        "bit_identical": {"b_vs_a": bool(torch.equal(last["b_kernel"], last["a_composed"])), "c_vs_a": bool(torch.equal(last["c_kernel_graphed"], last["a_composed"])),
                          "gate_c_vs_gate_a": bool(torch.equal(last["gate_c_kernel_graphed"], last["gate_a_composed"]))},
        "device": torch.cuda.get_device_name(0), "env": clock}
text = json.dumps(line)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
