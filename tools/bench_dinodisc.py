#!/usr/bin/env python
"""Times DinoDisc (--disc_type dino) at the production shape on one MI355X: ViT-S/14 with random weights, 256 px images, ks = 9.

    python tools/bench_dinodisc.py [--config bn|scripts] [--iters 10] [--repeats 3] [--depth 12]

  --config bn        the module's own defaults: BatchNormLocal, spectral norm, four taps (2, 5, 8, 11)
  --config scripts   what the trainers build (train_tokenizer.py:48-49,307-314): SyncBatchNorm ("sbn"), no spectral norm, five taps (0, 2, 5, 8, 11)

Two workloads, as the trainers run them (dmvae_amd/losses.py):
  disc_turn   the discriminator's turn: two train-mode passes over 64 images ([images; recon] at batch 32, twice) and the backward of a hinge + consistency loss
              to the heads' parameters (no image gradient)
  gen_term    the generator's adversarial term: 32 images, eval mode, frozen heads, backward to the image
each on the HIP route (`DinoDisc.forward`) and on the module's own plain-PyTorch statement (`forward_stock`, ATen / library kernels) under the same
autocast(bfloat16), in the same process, alternating, `--repeats` times so that the spread shows.  With `--config scripts` the generator's term is also timed on
route `composed`: the HIP route with the eval-mode head composed from the existing ops instead of `functional.DinoHeadEvalFn` -- plain `conv_tokens`,
`groupnorm_apply` with the running estimates as constant statistics, `groupnorm_bwd_apply` with zero sums (`functional.DinoHeadFn` handed
`models.patchgan._bn_stats` of an eval-mode norm) -- the alternative the fused epilogue and `dino_bnact_bwd` are measured against.  A time is the mean over
`--iters` calls between two device events after a warm-up of the same shape.  Prints one JSON line per (workload, route, repeat) and a summary line per workload."""
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
    ap.add_argument("--config", choices=("bn", "scripts"), default="bn")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dinodisc: needs a GPU (no CPU timing)")
    from dmvae_amd.models import dinodisc as D
    from dmvae_amd.models.dinodisc import DinoDisc
    torch.manual_seed(0)
    scripts = a.config == "scripts"
    taps = (0, 2, 5, 8, 11) if scripts else (2, 5, 8, 11)
    kw = dict(norm_type="sbn", norm_eps=1e-6, use_specnorm=False) if scripts else {}
    D.enable_syncbn_heads(scripts)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        disc = DinoDisc(9, "cuda", None, dino_depth=a.depth, key_depths=tuple(k for k in taps if k < a.depth) or (a.depth - 1,), **kw).cuda()
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

    def forward_composed(x):
        """`DinoDisc.forward` on the HIP route with every head through DinoHeadFn and the norms' own (eval-mode: constant) statistics."""
        from functools import partial
        from dmvae_amd.functional import DinoHeadFn
        from dmvae_amd.models.patchgan import _bn_stats
        from dmvae_amd.models.vit_fast import frozen_forward_features, frozen_taps_with_input_grad
        vit = disc.dino[0]
        x = disc.preprocess(x)
        pos = vit.pos_for(x.shape[-2], x.shape[-1])
        feats = (frozen_taps_with_input_grad if torch.is_grad_enabled() and x.requires_grad else frozen_forward_features)(vit, x, disc.key_depths, pos)
        out = []
        for head, t in zip(disc.heads, feats):
            c0, n0, c1, n1, c2 = head[0][0], head[0][1], head[1].fn[0], head[1].fn[1], head[2]
            cfg = (1, t.shape[-1], n0.eps, (partial(_bn_stats, n0), partial(_bn_stats, n1)))
            out.append(DinoHeadFn.apply(t, cfg, c0.weight_orig, c0.sigma(), c0.bias, n0.weight, n0.bias, c1.weight_orig, c1.sigma(), c1.bias, n1.weight, n1.bias,
                                        c2.weight_orig, c2.sigma(), c2.bias).view(x.shape[0], -1))
        return torch.cat(out, dim=1)

    routes = {"hip": disc.forward, "stock": disc.forward_stock}
    med = lambda v: sorted(v)[len(v) // 2]
    for name, fn in (("disc_turn", disc_turn), ("gen_term", gen_term)):
        rts = dict(routes, composed=forward_composed) if scripts and name == "gen_term" else routes
        ms = {r: [] for r in rts}
        for rep in range(a.repeats):
            for r, fwd in rts.items():
                t = timed(fn, fwd)
                ms[r].append(t)
                print(json.dumps({"workload": name, "config": a.config, "route": r, "repeat": rep, "ms": round(t, 3), "batch": a.batch, "px": a.px, "depth": a.depth,
                                  "iters": a.iters}), flush=True)
        hip, stock = med(ms["hip"]), med(ms["stock"])
        print(f"# {name} [{a.config}]: HIP {hip:.2f} ms (min {min(ms['hip']):.2f}, max {max(ms['hip']):.2f}), stock {stock:.2f} ms (min {min(ms['stock']):.2f}, "
              f"max {max(ms['stock']):.2f}); HIP / stock = {hip / stock:.3f}", flush=True)
        if "composed" in ms:
            comp = med(ms["composed"])
            print(f"# {name} [{a.config}]: eval head fused {hip:.2f} ms (min {min(ms['hip']):.2f}, max {max(ms['hip']):.2f}), composed {comp:.2f} ms "
                  f"(min {min(ms['composed']):.2f}, max {max(ms['composed']):.2f}); fused / composed = {hip / comp:.3f}", flush=True)


if __name__ == "__main__":
    main()
