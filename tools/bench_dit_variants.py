#!/usr/bin/env python
"""LightningDiT block variants, HIP route against the stock modules in one process: LightningDiT-XL/1 geometry (width 1152, 16 heads, depth 28, 256 tokens of a
32 x 16 x 16 latent) in two non-default configurations of the constructor's switches --

  plain : LayerNorm + GELU-MLP, no RoPE, no QK-norm (the original DiT / SiT block),
  noqk  : the default block without QK-norm,

at B = 16 under autocast(bf16), two cases each: the inference forward (frozen weights, no gradient: lightningdit_fast.forward_inference) and forward + backward
(trainable weights: lightningdit_fast.forward_train, one functional.DitBlockFn per block), each against the SAME model's `forward_stock` (ATen / library kernels) under the
same autocast.  The yardstick is the stock route on the same box in the same process, not an earlier run of this code.  The two routes alternate within every
round after one untimed round; a round times `--iters` calls between two device events.  Prints one JSON line per configuration: milliseconds per call (median
over the rounds, and every round), the spread of each series ((max - min) / median), the ratio HIP / stock, whether the gap exceeds both spreads, the rel-L2
distance of the two routes' outputs, and the device clock during the timed region.  Random weights: the time does not depend on them.

  python tools/bench_dit_variants.py [--rounds 5] [--iters 10] [--batch 16] [--out FILE]"""
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
from dmvae_amd.models.lightningdit import LightningDiT

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--depth", type=int, default=28)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_dit_variants.py measures on the GPU"

BF = torch.bfloat16
XL1 = dict(input_size=16, patch_size=1, in_channels=32, hidden_size=1152, depth=args.depth, num_heads=16, num_classes=1000)
CONFIGS = {"plain": dict(use_qknorm=False, use_swiglu=False, use_rope=False, use_rmsnorm=False, wo_shift=False), "noqk": dict(use_qknorm=False)}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


lines = []
for name, switches in CONFIGS.items():
    torch.manual_seed(0)
    m = LightningDiT(**XL1, **switches).cuda().eval()
    with torch.no_grad():
        for blk in m.blocks:                                             # the reference zero-initialises these: give the blocks something to do
            blk.adaLN_modulation[1].weight.normal_(0, 0.02)
            blk.adaLN_modulation[1].bias.normal_(0, 0.3)
        m.final_layer.linear.weight.normal_(0, 0.02)
        m.final_layer.adaLN_modulation[1].bias.normal_(0, 0.3)
    assert fast.variant_supported(m) and not fast.structurally_supported(m)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(args.batch, 32, 16, 16, generator=g).cuda()
    t, y = torch.rand(args.batch, generator=g).cuda(), torch.randint(0, 1001, (args.batch,), generator=g).cuda()
    dy = torch.randn(args.batch, 32, 16, 16, generator=g).cuda()
    out = {}

    def infer(route):
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            out["inf_" + route] = m(x, t, y) if route == "hip" else m.forward_stock(x, t, y)

    def train(route):
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF):
            o = m(x, t, y) if route == "hip" else m.forward_stock(x, t, y)
        (o.float() * dy).sum().backward()
        out["train_" + route] = o.detach()

    series = {k: [] for k in ("infer_hip", "infer_stock", "train_hip", "train_stock")}
    m.requires_grad_(False)
    with torch.autocast("cuda", dtype=BF):
        assert m._takes_inference_route(x), "the inference case must run lightningdit_fast.forward_inference"
    for route in ("hip", "stock"):                                       # the untimed round: every shape, both routes, both cases
        infer(route)
    m.requires_grad_(True)
    m.pos_embed.requires_grad_(False)
    for route in ("hip", "stock"):
        train(route)
    env = GpuEnvSampler(0)
    env.start()
    for _ in range(args.rounds):
        m.requires_grad_(False)
        for route in ("hip", "stock"):
            series["infer_" + route].append(timed(lambda: infer(route), args.iters))
        m.requires_grad_(True)
        m.pos_embed.requires_grad_(False)
        for route in ("hip", "stock"):
            series["train_" + route].append(timed(lambda: train(route), args.iters))
    clock = env.stop()
    med = {k: statistics.median(v) for k, v in series.items()}
    rl2 = lambda a, b: float(((a.double() - b.double()).norm() / b.double().norm()).item())
    line = {"bench": "dit_variants", "config": name, "switches": switches, "geometry": "LightningDiT-XL/1, 256 tokens", "depth": args.depth, "batch": args.batch,
            "rounds": args.rounds, "iters": args.iters,
            "ms": {k: round(v, 4) for k, v in med.items()}, "ms_rounds": {k: [round(x_, 4) for x_ in v] for k, v in series.items()},
            "spread": {k: round(spread(v), 5) for k, v in series.items()},
            "ratio_hip_over_stock": {c: round(med[c + "_hip"] / med[c + "_stock"], 5) for c in ("infer", "train")},
            # faster than stock by more than the spread of the repeats: the slowest HIP round under the fastest stock round
            "faster_beyond_spread": {c: bool(max(series[c + "_hip"]) < min(series[c + "_stock"])) for c in ("infer", "train")},
            "rel_l2_hip_vs_stock": {"infer": round(rl2(out["inf_hip"], out["inf_stock"]), 6), "train_out": round(rl2(out["train_hip"], out["train_stock"]), 6)},
            "device": torch.cuda.get_device_name(0), "env": clock}
    text = json.dumps(line)
    print(text, flush=True)
    lines.append(text)
    del m
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
