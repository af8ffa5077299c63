#!/usr/bin/env python
"""The Heun step and the "Tweedie" / "Euler" last steps of the SDE sampler, kernel route against the tensor-op composition of the same tree, in one process:
LightningDiT-XL/1 at sample_50k's batch (n = 25 latents of 32 x 16 x 16) under autocast(bf16), the DiT forward as one hipGraph replay per evaluation on both
routes (what `SamplePipeline` runs), so the routes differ in the state update and the time vectors only:

  heun      `sample_sde(sampling_method="Heun")` over `--steps` sampler steps -- all but the last are Heun steps (two evaluations + `ops.sde_heun_perturb /
            _predict / _correct`, against the reference's ~25 elementwise launches and its pageable host-to-device copies of the time vectors), the last is the
            "Mean" step --: ms per sampler step,
  tweedie   the "Tweedie" last step alone (`Sampler._last_step`: one evaluation + `ops.sde_last_step`), ms per call,
  euler     the "Euler" last step alone, ms per call.

With `--prediction noise` or `score` the model's output is read as the noise / the score (`create_transport(path_type, prediction, None, 1e-3, 1e-3)`): the
kernel route is then the `_m` kernels, which convert the output to the velocity inside each pass, and two more items are timed:

  em        `sample_sde(sampling_method="Euler")` over `--steps` sampler steps (one evaluation + `ops.sde_euler_step_m` each), ms per sampler step,
  drift     one evaluation of the probability-flow ODE's drift as dopri5 takes it -- the forward and `ops.model_velocity` into a stage buffer, against
            `Transport.get_drift`'s composition and the solver's copy into the buffer --, ms per evaluation.

The defaults (`--path_type Linear --prediction velocity`) are the run described above; `--path_type GVP` or `VP` selects the curved paths (the tool turns
`transport.enable_all_paths` on itself).

`transport.FUSED_STATE_UPDATE` selects the route.  The routes alternate within every round after one untimed round; each run is timed with device events around
the whole call.  Prints one JSON line: milliseconds per step / call (median over the rounds, and every round), the run-to-run spread of each composed route
((max - min) / median over its rounds), the ratio fused / composed, whether the fused route is not slower than the composed one beyond that spread, whether the
two routes' results are bit-identical (and how far apart they are), and the device clock during the timed region.  Random DiT weights: the times do not depend
on them.  The Heun runs need not be bit-identical: the composition takes sqrt(2 diffusion) with ATen's device sqrt, which on this stack is not correctly rounded
(one f32 input in six is an ulp away from the host's), the kernel route takes the host's, as the CPU reference does; the trajectories part at the first step whose
coefficient is such an input.

  python tools/bench_sampler_methods.py [--steps 40] [--calls 40] [--rounds 4] [--n 25] [--path_type Linear] [--prediction velocity|noise|score] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from bench import GpuEnvSampler
from dmvae_amd import transport as T
from dmvae_amd.models import lightningdit_fast as fast
from dmvae_amd.models.lightningdit import LightningDiT_models

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40, help="sampler steps per timed Heun run")
ap.add_argument("--calls", type=int, default=40, help="last-step calls per timed run")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--n", type=int, default=25)
ap.add_argument("--path_type", default="Linear")
ap.add_argument("--prediction", default="velocity", choices=["velocity", "noise", "score"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_sampler_methods.py measures on the GPU"

BF = torch.bfloat16
torch.manual_seed(0)
dit = LightningDiT_models["LightningDiT-XL/1"](input_size=16, in_channels=32, num_classes=1000).cuda().eval().requires_grad_(False)
with torch.no_grad():
    for blk in dit.blocks:
        blk.adaLN_modulation[1].weight.normal_(0, 0.02)
    dit.final_layer.linear.weight.normal_(0, 0.02)
z = torch.randn(args.n, 32, 16, 16, device="cuda")
y = torch.randint(0, 1000, (args.n,), device="cuda")
MODEL_OUT = args.prediction != "velocity"           # a noise / score model: eps as the reference's drivers default them for it
T.enable_all_paths()                                # --path_type GVP | VP: the tool asks for the plans itself
sampler = T.Sampler(T.create_transport(args.path_type, args.prediction, None, 1e-3, 1e-3) if MODEL_OUT or args.path_type != "Linear" else T.create_transport())
heun_fn = sampler.sample_sde(sampling_method="Heun", diffusion_form="sigma", last_step="Mean", last_step_size=0.04, num_steps=args.steps)
LAST_SIZE = 0.04
sde_drift, _ = sampler._sde_diffusion_and_drift(diffusion_form="sigma", diffusion_norm=1.0)
fused_arg = (sampler.transport.path_sampler, "sigma", 1.0, sampler.transport.model_type)
last_fns = {name: sampler._last_step(sde_drift, last_step=name, last_step_size=LAST_SIZE, t1=1 - LAST_SIZE, fused=fused_arg) for name in ("Tweedie", "Euler")}
t_last = torch.ones(args.n, device="cuda") * (1 - LAST_SIZE)
with torch.no_grad(), torch.autocast("cuda", dtype=BF):
    model = fast.GraphedInference(dit, z, torch.zeros(args.n, device="cuda"), y)


def timed(fn, per):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        b.synchronize()
    return a.elapsed_time(b) / per, out.clone()


def run_heun():
    torch.manual_seed(1)                                             # the same noise stream for both routes
    return timed(lambda: heun_fn(z, model, y=y)[-1], args.steps)


def run_last(name):
    def calls():
        for _ in range(args.calls):
            out = last_fns[name](z, t_last, model, y=y)              # always from z: the same work every call
        return out
    return timed(calls, args.calls)


items = [("heun", run_heun), ("tweedie", lambda: run_last("Tweedie")), ("euler", lambda: run_last("Euler"))]
if MODEL_OUT:
    em_fn = sampler.sample_sde(sampling_method="Euler", diffusion_form="sigma", last_step="Mean", last_step_size=0.04, num_steps=args.steps)
    ode_fn = sampler.sample_ode(sampling_method="dopri5")
    _ode, stage = ode_fn.__self__, torch.empty_like(z)
    T_DRIFT = 0.5139

    def run_em():
        torch.manual_seed(1)
        return timed(lambda: em_fn(z, model, y=y)[-1], args.steps)

    def run_drift():
        tv = torch.full((args.n,), T_DRIFT, device="cuda")

        def calls():
            for _ in range(args.calls):
                if T.FUSED_STATE_UPDATE:
                    _ode._velocity_into(T_DRIFT, tv, z, stage, model, dict(y=y))
                else:
                    stage.copy_(sampler.drift(z, tv, model, y=y))
            return stage
        return timed(calls, args.calls)

    items += [("em", run_em), ("drift", run_drift)]
routes = [(f"{item}_{'fused' if fused else 'composed'}", fn, fused) for item, fn in items for fused in (True, False)]
times, last = {name: [] for name, *_ in routes}, {}


def run(fn, fused):
    T.FUSED_STATE_UPDATE = fused
    try:
        return fn()
    finally:
        T.FUSED_STATE_UPDATE = True


for name, fn, fused in routes:                                       # the untimed round: every route
    run(fn, fused)
env = GpuEnvSampler(0)
env.start()
for _ in range(args.rounds):
    for name, fn, fused in routes:
        ms, last[name] = run(fn, fused)
        times[name].append(ms)
clock = env.stop()
med = {k: statistics.median(v) for k, v in times.items()}
line = {"bench": "sampler_methods", "model": "LightningDiT-XL/1", "path_type": args.path_type, "prediction": args.prediction, "n": args.n, "heun_steps": args.steps, "last_step_calls": args.calls, "rounds": args.rounds,
        "ms": {k: round(v, 4) for k, v in med.items()}, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in times.items()}}
for item, _ in items:
    c = times[f"{item}_composed"]
    spread = (max(c) - min(c)) / med[f"{item}_composed"]
    ratio = med[f"{item}_fused"] / med[f"{item}_composed"]
    f, c = last[f"{item}_fused"], last[f"{item}_composed"]
    line[item] = {"spread_composed": round(spread, 5), "ratio_fused_over_composed": round(ratio, 5), "fused_not_slower_beyond_spread": bool(ratio <= 1 + spread),
                  "bit_identical": bool(torch.equal(f, c)), "max_abs_diff_over_max_abs": float((f - c).abs().max() / c.abs().max())}
line.update(device=torch.cuda.get_device_name(0), env=clock)
text = json.dumps(line)
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
