#!/usr/bin/env python
"""Sampler.sample_ode_likelihood at its defaults (dopri5, atol 1e-6 / rtol 1e-3, num_steps 50) with LightningDiT-XL/1 at sample_50k's batch (25 latents of
32 x 16 x 16) under autocast(bf16): model evaluations, accepted / rejected steps, wall time per batch and logp in bits/dim of the DiT's input space; then the
cost of ONE evaluation -- the forward whose graph gives the VJP, the input-VJP of the frozen model (dx-only backward), and for comparison the reference's
structure (two forwards plus the full training backward with every weight gradient, which the trainable route times).  Random DiT weights: the velocity
field is not a trained model's, so the NFE and the bits/dim are not what a trained checkpoint gives -- the per-evaluation costs carry over.

  python tools/bench_ode_likelihood.py                       # the timed batch and the per-evaluation costs
  python tools/bench_ode_likelihood.py --analyze TRACE.csv   # rocprofv3 --kernel-trace output of one run (SOLVE_ONLY=1): integrator + pack kernel share

B env changes the batch; SOLVE_ONLY=1 runs one solve only (for the profiler)."""
import csv, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def analyze(path):
    rows = list(csv.DictReader(open(path)))
    ks = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows]
    total = sum(e - s for s, e, _ in ks)
    pack = sum(e - s for s, e, n in ks if "ode_hutchinson_pack" in n)
    integ = sum(e - s for s, e, n in ks if "dmvae_sampler::ode_" in n and "ode_hutchinson_pack" not in n)
    npack = sum(1 for *_, n in ks if "ode_hutchinson_pack" in n)
    dx = sum(e - s for s, e, n in ks if "<true, true, false>" in n or "<true, false, false>" in n or "<false, true, false>" in n or "_bwd_kernel<false>" in n)
    print(f"kernels {len(ks)}, device time {total / 1e6:.2f} ms; dopri5 kernels (ode_rk_combine / ode_err_* / ode_dense) {integ / 1e6:.3f} ms = "
          f"{100 * integ / total:.3f} %; Hutchinson pack {npack} launches {pack / 1e6:.3f} ms = {100 * pack / total:.3f} %; "
          f"dx-only boundary / QK-norm kernels {dx / 1e6:.3f} ms = {100 * dx / total:.2f} % of device time")


if len(sys.argv) > 2 and sys.argv[1] == "--analyze":
    analyze(sys.argv[2])
    sys.exit(0)

import copy
import numpy as np
import torch
from dmvae_amd.models.lightningdit import LightningDiT_models
from dmvae_amd.transport import Sampler, create_transport

N = int(os.environ.get("B", "25"))
BF = torch.bfloat16
torch.manual_seed(0)
dit = LightningDiT_models["LightningDiT-XL/1"](input_size=16, in_channels=32, num_classes=1000).cuda().eval()
with torch.no_grad():
    for blk in dit.blocks:
        blk.adaLN_modulation[1].weight.normal_(0, 0.02)
    dit.final_layer.linear.weight.normal_(0, 0.02)
frozen = copy.deepcopy(dit).requires_grad_(False)
x = torch.randn(N, 32, 16, 16, device="cuda") * 0.5; y = torch.randint(0, 1000, (N,), device="cuda")
fn = Sampler(create_transport()).sample_ode_likelihood()
with torch.autocast("cuda", dtype=BF):
    torch.manual_seed(1)
    if os.environ.get("SOLVE_ONLY") != "1":
        fn(x[:2], frozen.forward, y=y[:2])                         # one-off per shape: weight caches, outside the timed batch
    torch.cuda.synchronize(); t0 = time.perf_counter()
    logp, z = fn(x, frozen.forward, y=y)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
o = fn.ode
bpd = (-logp / x[0].numel() / np.log(2)).cpu()
print(f"likelihood dopri5, batch {N}: {dt:.2f} s / batch; NFE {o.nfe} (accepted {o.n_accepted}, rejected {o.n_rejected}), {dt / o.nfe * 1e3:.2f} ms / evaluation; "
      f"bits/dim mean {bpd.mean().item():.4f} (min {bpd.min().item():.4f}, max {bpd.max().item():.4f}); logp finite {bool(torch.isfinite(logp).all())}", flush=True)
if os.environ.get("SOLVE_ONLY") == "1":
    sys.exit(0)


def timed(f, reps=10):
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / reps


t = torch.full((N,), 0.5, device="cuda")
eps = torch.randint(2, x.size(), dtype=torch.float, device="cuda") * 2 - 1
state = {}


def fwd():
    xr = x.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        state["xr"], state["v"] = xr, frozen(xr, t, y)


def vjp():
    with torch.autocast("cuda", dtype=BF):
        torch.autograd.grad((state["v"] * eps).sum(), state["xr"])


def fwd_vjp():
    fwd(); vjp()


def reference_structure():                                          # transport.py:420-428: forward + full backward, then the second forward
    xr = x.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        v = dit(xr, t, y)
        torch.autograd.grad((v * eps).sum(), xr)                     # trainable weights: the existing route computes every weight gradient
        dit(xr, t, y)
    for p in dit.parameters():
        p.grad = None


t_fwd = timed(fwd)
t_both = timed(fwd_vjp)
t_ref = timed(reference_structure)
with torch.no_grad(), torch.autocast("cuda", dtype=BF):
    t_inf = timed(lambda: frozen(x, t, y))
print(f"per evaluation at batch {N}: graph-building forward {t_fwd:.2f} ms + input-VJP (dx only) {t_both - t_fwd:.2f} ms = {t_both:.2f} ms; "
      f"reference structure (forward + full training backward + second forward) {t_ref:.2f} ms -> {t_ref / t_both:.2f}x; "
      f"inference forward for scale {t_inf:.2f} ms", flush=True)
