#!/usr/bin/env python
"""Times the reference's OWN training loop (train_tokenizer.py:403-437) over dmvae_amd's VAE + LPIPS + losses on one MI355X, with three optimiser tails.

    python tools/bench_reference_loop.py [--batch 32] [--px 256] [--model_size large] [--iters 10] [--warmup 3] [--repeats 3]

The loop is the scripts', statement for statement: autocast(bfloat16) around forward, the loss with its four `.item()` reads (forward_generator, :180-189),
backward, `clip_grad_norm_(...).item()`, `optimizer.step()`, `zero_grad(set_to_none=True)`, `LambdaLR.step()`; then `update_ema` on a deepcopy of the model.
No TokenizerTrainer, no flat buffers: this is what someone who runs the unedited script through run_on_mi355x.py gets.  The tails:

  stock       torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ + the scripts' Python update_ema loop      (the drop-in user's tail without --hip-optim)
  hip_optim   dmvae_amd.optim.AdamW + clip_grad_norm_, the scripts' Python update_ema loop                  (what --hip-optim gives an unedited script)
  hip_all     hip_optim + dmvae_amd.optim.update_ema                                                        (the one-line import on top)

All three run in one process on the same model, in interleaved rounds (stock, hip_optim, hip_all, stock, ...), `--repeats` rounds, so that drift of the box shows
as spread instead of as a difference.  A time is the wall-clock mean over `--iters` steps between two device synchronisations (the loop syncs on every `.item()`,
so host time is part of the step), after `--warmup` steps of the same tail.  Launches per step are counted from one profiled step per tail (kernel records of
torch.profiler); null when the profiler is not available.  Prints one JSON line per (tail, round) and one summary line per tail."""
import argparse
import copy
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

TAILS = ("stock", "hip_optim", "hip_all")


def python_update_ema(ema_model, model, decay=0.9999):
    """train_tokenizer.py:140-150"""
    with torch.no_grad():
        ema_params = dict(ema_model.named_parameters())
        for name, param in model.named_parameters():
            ema_params[name].mul_(decay).add_(param.data, alpha=1 - decay)


class Loop:
    def __init__(self, tail, vae, lpips, images, lr=1e-4, warmup_steps=1000):
        from dmvae_amd import optim
        hip = tail != "stock"
        self.vae, self.lpips, self.images = vae, lpips, images
        adamw = optim.AdamW if hip else torch.optim.AdamW
        self.clip = optim.clip_grad_norm_ if hip else torch.nn.utils.clip_grad_norm_
        self.update_ema = optim.update_ema if tail == "hip_all" else python_update_ema
        self.opt = adamw([p for p in vae.parameters() if p.requires_grad], lr=lr, weight_decay=0.005, betas=(0.9, 0.95), eps=1e-8)      # :381-382
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda s: s / warmup_steps if s < warmup_steps else 1.0)              # :385-391
        self.ema_model = copy.deepcopy(vae).requires_grad_(False).eval()                                                               # :397-399
        self.log = {}

    def step(self):
        from dmvae_amd import losses
        vae, x = self.vae, self.images
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):                      # :410
            recon = vae(x, return_latent=False)
            l1, l2 = losses.l1_mse(recon, x, 1.0, 0.0)                                      # forward_generator, :180-183 (args.l1 = 1, args.l2 = 0, args.lpips = 1)
            lp = self.lpips(x, recon).mean()
            rec_loss = l1 * 1.0 + l2 * 0.0 + lp * 1.0
            self.log = {"L1": l1.detach().item(), "L2": l2.detach().item(), "LPIPS": lp.detach().item(), "rec_loss": rec_loss.detach().item()}
            rec_loss.mean().backward()
            self.log["vae_norm"] = self.clip(vae.parameters(), max_norm=1.0).item()         # :415-416
            self.opt.step()
            self.opt.zero_grad(set_to_none=True)
            self.sched.step()
        self.update_ema(self.ema_model, vae)                                                # :437


def count_launches(loop):
    """Kernel records of one whole step (forward, backward and tail; copies and memsets left out).  The tails share forward and backward, so the difference
    between two tails' counts is the difference between their tails."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            loop.step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as e:           # no tracer on this box: stated, not guessed
        print(f"# launch count unavailable: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--px", type=int, default=256)
    ap.add_argument("--model_size", default="large")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-launch-count", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reference_loop: needs a GPU (no CPU timing)")
    from dmvae_amd.models.vae import VAE
    from dmvae_amd.utils.lpips import LPIPS
    torch.manual_seed(42)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # random weights: nothing to download offline
        vae = VAE(z_channels=32, model_size=a.model_size).cuda()
        lpips = LPIPS().eval().requires_grad_(False).cuda()
    with torch.no_grad():
        for lin in (lpips.lin0, lpips.lin1, lpips.lin2, lpips.lin3, lpips.lin4):
            lin.model[-1].weight.fill_(1.0 / lin.model[-1].weight.shape[1])
    vae.encoder.eval()
    vae.encoder.requires_grad_(False)                                                       # :295-297
    images = torch.rand(a.batch, 3, a.px, a.px, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 2 - 1
    n_tensors = sum(1 for _ in vae.parameters())
    n_train = sum(1 for p in vae.parameters() if p.requires_grad)
    loops = {t: Loop(t, vae, lpips, images) for t in TAILS}
    times = {t: [] for t in TAILS}
    for r in range(a.repeats):
        for t in TAILS:
            loop = loops[t]
            for _ in range(a.warmup):
                loop.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                loop.step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.iters
            times[t].append(ms)
            print(json.dumps({"tail": t, "round": r, "ms_per_step": round(ms, 3), "rec_loss": loop.log["rec_loss"], "vae_norm": loop.log["vae_norm"]}), flush=True)
    base = sum(times["stock"]) / len(times["stock"])
    for t in TAILS:
        v = times[t]
        mean = sum(v) / len(v)
        launches = None if a.no_launch_count else count_launches(loops[t])
        print(json.dumps({"summary": t, "batch": a.batch, "px": a.px, "model_size": a.model_size, "tensors": n_tensors, "trainable_tensors": n_train,
                          "ms_per_step_mean": round(mean, 3), "ms_per_step_min": round(min(v), 3), "ms_per_step_max": round(max(v), 3),
                          "spread_pct": round(100 * (max(v) - min(v)) / min(v), 2), "vs_stock_ms": round(mean - base, 3),
                          "kernel_launches_per_step": launches}), flush=True)


if __name__ == "__main__":
    main()
