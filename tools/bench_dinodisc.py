#!/usr/bin/env python
"""Times DinoDisc (--disc_type dino) at the production shape on one MI355X: ViT-S/14 with random weights, 256 px images, ks = 9, four heads.

    python tools/bench_dinodisc.py [--iters 10] [--repeats 3] [--depth 12]

Two workloads, as the trainers run them (dmvae_amd/losses.py):
  disc_turn   the discriminator's turn: two train-mode passes over 64 images ([images; recon] at batch 32, twice) and the backward of a hinge + consistency loss
              to the heads' parameters (no image gradient)
  gen_term    the generator's adversarial term: 32 images, eval mode, frozen heads, backward to the image
each on the HIP route (`DinoDisc.forward`) and on the module's own plain-PyTorch statement (`forward_stock`, ATen / library kernels) under the same
autocast(bfloat16), in the same process, alternating, `--repeats` times so that the spread shows.  A time is the mean over `--iters` calls between two device
events after a warm-up of the same shape.  Prints one JSON line per (workload, route, repeat) and a summary line per workload."""
import argparse
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--px", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dinodisc: needs a GPU (no CPU timing)")
    from dmvae_amd.models.dinodisc import DinoDisc
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        disc = DinoDisc(9, "cuda", None, dino_depth=a.depth, key_depths=tuple(k for k in (2, 5, 8, 11) if k < a.depth) or (a.depth - 1,)).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    both1 = torch.rand(2 * a.batch, 3, a.px, a.px, device="cuda", generator=g) * 2 - 1
    both2 = torch.rand(2 * a.batch, 3, a.px, a.px, device="cuda", generator=g) * 2 - 1
    xg = torch.rand(a.batch, 3, a.px, a.px, device="cuda", generator=g) * 2 - 1

    def disc_turn(fwd):
        disc.train().requires_grad_(True)
        for p in disc.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            l1 = fwd(both1).float()
            l2 = fwd(both2).float()
            loss = 0.5 * (torch.relu(1 - l1[:a.batch]).mean() + torch.relu(1 + l1[a.batch:]).mean()) + torch.nn.functional.mse_loss(l2, l1)
        loss.backward()

    def gen_term(fwd):
        disc.eval().requires_grad_(False)
        x = xg.detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            gl = -fwd(x).float().mean()
        torch.autograd.grad(gl, x)

    def timed(fn, fwd):
        fn(fwd)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn(fwd)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    routes = {"hip": disc.forward, "stock": disc.forward_stock}
    for name, fn in (("disc_turn", disc_turn), ("gen_term", gen_term)):
        ms = {r: [] for r in routes}
        for rep in range(a.repeats):
            for r, fwd in routes.items():
                t = timed(fn, fwd)
                ms[r].append(t)
                print(json.dumps({"workload": name, "route": r, "repeat": rep, "ms": round(t, 3), "batch": a.batch, "px": a.px, "depth": a.depth, "iters": a.iters}), flush=True)
        hip, stock = sorted(ms["hip"])[len(ms["hip"]) // 2], sorted(ms["stock"])[len(ms["stock"]) // 2]
        print(f"# {name}: HIP {hip:.2f} ms (min {min(ms['hip']):.2f}, max {max(ms['hip']):.2f}), stock {stock:.2f} ms (min {min(ms['stock']):.2f}, "
              f"max {max(ms['stock']):.2f}); HIP / stock = {hip / stock:.3f}", flush=True)


if __name__ == "__main__":
    main()
