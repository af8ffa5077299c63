#!/usr/bin/env python
"""Times dmvae_amd.models.lpips_alex.LPIPSAlex on one MI355X against the same module's stock f32 composition, on the same device, in the same process.

    python tools/bench_lpips_eval.py [--pairs 32,128] [--size 256] [--iters 5] [--rounds 3] [--out FILE]

  hip     `forward` on the kernels of csrc/inception.hip (exact f32 on v_mfma_f32_16x16x4_f32) and csrc/lpips_eval.hip (input pass, f64 head), f32
          [P, 3, S, S] pairs in, range check off (it is one host synchronisation and not part of either route).
  stock   `forward_stock` of the same module with the same parameters: F.conv2d / F.relu / F.max_pool2d and the library's f32 head arithmetic on device
          tensors.

Parameters are seeded random values (the published weights are not on this machine); times do not depend on them.  Rounds are interleaved: every round
times both routes, one after the other.  A time is the mean over `--iters` calls between two device events after a warm-up call of the same shape; the
table gives the median and the spread over the rounds.  The trunk's rate is the five convolutions' 2 Ho Wo Cout Cin k k flops for both images of a pair,
over the whole call's time: a whole-network rate, not a kernel's share of peak.
  The head is then timed alone, level by level, on the taps of the same images: `ops.lpips_head` calls back to back between two device events (each call is
the reduction launch, the per-pair finalize launch and the workspace allocation).  Its algorithmic bytes are the features it must read once,
2 P h w c x 4 B (lin and the P results are noise), and the rate printed is those bytes over the call time -- to be read against the 6.3 TB/s a streaming
read of HBM reaches on this device and, for a tap that fits the 256 MiB Infinity Cache (the repeated calls then re-read it from there), against nothing
in particular: the line says which case a level is.  No CPU timing: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters                         # ms per call


def trunk_shapes(size):
    """-> [(h, w, c, conv flops per image)] per tap, by the layers' own shape arithmetic."""
    from dmvae_amd.models.lpips_alex import TRUNK
    out, h, w = [], size, size
    for _, _, cin, cout, k, stride, pad, pool in TRUNK:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        out.append((h, w, cout, 2 * h * w * cout * cin * k * k))
    return out


def random_parameters(net, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.convs():
            fan_in = m.weight[0].numel()
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
        for m in net.lins():
            m.weight.copy_(torch.rand(m.weight.shape, generator=g) / m.weight.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="32,128")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--head-iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lpips_eval: needs a GPU (no CPU timing)")
    from dmvae_amd import ops
    from dmvae_amd.models.lpips_alex import LPIPSAlex
    dev = "cuda:0"
    net = LPIPSAlex(chunk=128)
    random_parameters(net)
    net = net.to(dev)
    shapes = trunk_shapes(a.size)
    flops = 2 * sum(s[3] for s in shapes)                               # both images of a pair
    lines = [f"LPIPSAlex at {a.size} x {a.size}: {flops / 1e9:.3f} GFLOP per pair in the 2 x 5 convolutions; taps (h, w, c): {[s[:3] for s in shapes]}",
             f"device: {torch.cuda.get_device_name(0)}; iters {a.iters}, rounds {a.rounds}; times are medians over the rounds (min .. max)", ""]
    for p in (int(s) for s in a.pairs.split(",")):
        g = torch.Generator().manual_seed(p)
        x1 = (torch.rand(p, 3, a.size, a.size, generator=g) * 2 - 1).to(dev)
        x2 = (x1 + 0.2 * torch.randn(p, 3, a.size, a.size, generator=g).to(dev)).clamp(-1, 1)
        routes = {"hip": lambda: net(x1, x2, check_range=False), "stock": lambda: net.forward_stock(x1, x2)}
        v_hip, v_stock = routes["hip"](), routes["stock"]().double()
        dist = ((v_hip - v_stock).abs() / v_hip).max().item()
        times = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, fn in routes.items():
                times[k].append(timed(fn, a.iters))
        lines.append(f"P = {p} pairs   (mean value {v_hip.mean().item():.6e}; largest per-image relative distance between the routes' values: {dist:.2e})")
        for k, ts in times.items():
            med = statistics.median(ts)
            lines.append(f"  {k:6s} {med:9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})   {p / med * 1e3:9.1f} pairs/s   {flops * p / med / 1e9:7.2f} TFLOP/s f32 (whole call)")
        lines.append(f"  hip / stock time: {statistics.median(times['hip']) / statistics.median(times['stock']):.2f}")
        taps = net.taps(x1, x2, chunk=p)
        lins = net._operands(torch.device(dev))["lin"]
        out = torch.zeros(p, dtype=torch.float64, device=dev)
        total_head = 0.0
        lines.append(f"  the head alone, level by level ({a.head_iters} calls back to back; bytes = 2 P h w c x 4):")
        for level, (f, lin) in enumerate(zip(taps, lins)):
            ts = [timed(lambda: ops.lpips_head(f, lin, net.eps, out=out, accumulate=level > 0), a.head_iters) for _ in range(a.rounds)]
            med, nbytes = statistics.median(ts), f.numel() * 4
            total_head += med
            where = "fits the Infinity Cache: re-read from there" if nbytes < 200 * 2 ** 20 else "larger than the Infinity Cache: from HBM"
            lines.append(f"    level {level} {tuple(f.shape)}: {med * 1e3:8.1f} us ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f})  {nbytes / 2 ** 20:7.1f} MiB  "
                         f"{nbytes / med / 1e9:7.3f} TB/s  ({where})")
        lines.append(f"    five levels: {total_head:.3f} ms = {100 * total_head / statistics.median(times['hip']):.1f} % of the hip call")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
