#!/usr/bin/env python
"""sample_50k.py --mode ODE at its defaults (per_proc_batch_size 25, DiT-XL/1, time_dist_shift 2.5, dopri5 with atol 1e-6 / rtol 1e-3, num_steps 50):
model evaluations, accepted / rejected steps, wall time per batch and images/s of noise -> latents -> decode -> uint8 on the HIP path, next to SDE Euler-250
on the same box.  Random DiT weights: the velocity field is not a trained model's, so the NFE (and with it the wall time) is not what a trained
checkpoint takes -- the per-evaluation cost and the integrator's overhead are what carry over.

  python tools/bench_sample_ode.py                       # the timed batches
  python tools/bench_sample_ode.py --analyze TRACE.csv   # rocprofv3 --kernel-trace output of one run (ODE_ONLY=1): integrator share, readback gaps

STEPS env shortens the SDE arm; ODE_ONLY=1 skips it (one batch under the profiler)."""
import csv, os, sys, time, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def analyze(path):
    rows = list(csv.DictReader(open(path)))
    ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows), key=lambda r: r[0])
    total = sum(e - s for s, e, _ in ks)
    ode = sum(e - s for s, e, n in ks if "dmvae_sampler::ode_" in n)
    gaps, steps = [], []
    for i, (s, e, n) in enumerate(ks):
        if "ode_err_final_kernel" in n:
            j = i + 1
            while j < len(ks) and "copyBuffer" in ks[j][2]:         # the 8-byte device -> host copy runs as a blit kernel
                e = ks[j][1]
                j += 1
            if j < len(ks):
                gaps.append(ks[j][0] - e)                          # device idle: the host waits for the copy, decides, launches the next kernel
                steps.append(e)
    step_wall = [(b - a) for a, b in zip(steps, steps[1:])]
    gaps.sort()
    med = lambda v: sorted(v)[len(v) // 2] if v else float("nan")
    print(f"kernels {len(ks)}, device time {total / 1e6:.2f} ms; dopri5 kernels (ode_rk_combine / ode_err_* / ode_dense) {ode / 1e6:.3f} ms = "
          f"{100 * ode / total:.3f} % of device time")
    print(f"readbacks {len(gaps)}: idle gap after the readback copy median {med(gaps) / 1e3:.1f} us, max {max(gaps) / 1e3:.1f} us; "
          f"attempted step median {med(step_wall) / 1e6:.2f} ms -> gap / step {100 * med(gaps) / med(step_wall):.2f} %")


if len(sys.argv) > 2 and sys.argv[1] == "--analyze":
    analyze(sys.argv[2])
    sys.exit(0)

import torch
from dmvae_amd.models.lightningdit import LightningDiT_models
from dmvae_amd.models.vae import VAE
from dmvae_amd.sample import SamplePipeline

N = int(os.environ.get("B", "25")); STEPS = int(os.environ.get("STEPS", "250"))
torch.manual_seed(0)
dit = LightningDiT_models["LightningDiT-XL/1"](input_size=16, in_channels=32, num_classes=1000).cuda().eval().requires_grad_(False)
with torch.no_grad():
    for blk in dit.blocks:
        blk.adaLN_modulation[1].weight.normal_(0, 0.02)
    dit.final_layer.linear.weight.normal_(0, 0.02)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    vae = VAE(z_channels=32, model_size="large").cuda().eval().requires_grad_(False)
z = torch.randn(N, 32, 16, 16, device="cuda"); y = torch.randint(0, 1000, (N,), device="cuda")
kw = dict(latent_mean=0.0685, latent_scale=0.1763, time_dist_shift=2.5)
arms = [("ODE dopri5", SamplePipeline(dit, vae, mode="ODE", sampling_method="dopri5", num_sampling_steps=50, **kw))]
if os.environ.get("ODE_ONLY") != "1":
    arms.append((f"SDE Euler-{STEPS}", SamplePipeline(dit, vae, num_sampling_steps=STEPS, **kw)))
for name, pipe in arms:
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        pipe._model_fn(z, y)                                      # one-off per shape: weight caches + graph capture, outside the timed batch
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = pipe.images_uint8(z, y)[0].cpu()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    line = f"{name}: {dt:.2f} s / batch of {N} = {N / dt:.2f} images/s; out {tuple(out.shape)} {out.dtype}"
    o = getattr(pipe.sample_fn, "__self__", None)
    if name.startswith("ODE"):
        line += f"; NFE {o.nfe} (accepted {o.n_accepted}, rejected {o.n_rejected}), {dt / o.nfe * 1e3:.2f} ms / evaluation"
    else:
        line += f", {dt / STEPS * 1e3:.2f} ms / step"
    print(line, flush=True)
