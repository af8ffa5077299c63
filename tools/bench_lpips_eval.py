#!/usr/bin/env python
"""Times the evaluation LPIPS' networks (dmvae_amd.models.lpips_alex.LPIPSAlex, dmvae_amd.models.lpips_eval.LPIPSVGG / LPIPSSqueeze) on one MI355X against
the same module's stock f32 composition, on the same device, in the same process.

    python tools/bench_lpips_eval.py [--net alex|vgg|squeeze] [--pairs 32,128] [--size 256] [--iters 5] [--rounds 3] [--chunk N] [--out FILE]

  hip     `forward` on the kernels of csrc/inception.hip (exact f32 on v_mfma_f32_16x16x4_f32) and csrc/lpips_eval.hip (input pass, f64 head), f32
          [P, 3, S, S] pairs in, range check off (it is one host synchronisation and not part of either route).
  stock   `forward_stock` of the same module with the same parameters: F.conv2d / F.relu / F.max_pool2d and the library's f32 head arithmetic on device
          tensors.

Parameters are seeded random values (the published weights are not on this machine); times do not depend on them.  Rounds are interleaved: every round
times both routes, one after the other.  A time is the mean over `--iters` calls between two device events after a warm-up call of the same shape; the
table gives the median and the spread over the rounds.  The trunk's rate is the convolutions' 2 Ho Wo Cout Cin k k flops for both images of a pair (taken
from the module's own Conv2d layers by a shape-recording pass of the stock route), over the whole call's time: a whole-network rate, not a kernel's
share of peak.
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


def trunk_shapes(net, size):
    """-> ([(h, w, c)] per tap, conv flops per image): one CPU pass of the stock trunk on a zero image, every F.conv2d call recorded."""
    import torch.nn.functional as F
    flops, real = [0], F.conv2d

    def counting(x, w, *args, **kw):
        y = real(x, w, *args, **kw)
        flops[0] += 2 * y.shape[2] * y.shape[3] * w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3]
        return y
    F.conv2d = counting
    try:
        with torch.no_grad():
            taps = [(t.shape[2], t.shape[3], t.shape[1]) for t in net._stock_taps(torch.zeros(1, 3, size, size))]
    finally:
        F.conv2d = real
    return taps, flops[0]


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
    ap.add_argument("--net", default="alex", choices=("alex", "vgg", "squeeze"))
    ap.add_argument("--chunk", type=int, default=0, help="image pairs per pass of the network (0: 128 for alex and squeeze, 32 for vgg)")
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
    from dmvae_amd.models.lpips_eval import LPIPSSqueeze, LPIPSVGG
    dev = "cuda:0"
    cls = {"alex": LPIPSAlex, "vgg": LPIPSVGG, "squeeze": LPIPSSqueeze}[a.net]
    net = cls(chunk=a.chunk or (32 if a.net == "vgg" else 128))
    random_parameters(net)
    shapes, per_image = trunk_shapes(net, a.size)
    net = net.to(dev)
    flops = 2 * per_image                                               # both images of a pair
    lines = [f"{cls.__name__} at {a.size} x {a.size}, chunk {net.chunk}: {flops / 1e9:.3f} GFLOP per pair in the 2 x {len(net.convs())} convolutions; "
             f"taps (h, w, c): {shapes}",
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
        taps = net.taps(x1[:net.chunk], x2[:net.chunk])                       # one chunk's taps: what one head call of the network sees
        hp = taps[0].shape[0] // 2
        lins = net._operands(torch.device(dev))["lin"]
        out = torch.zeros(hp, dtype=torch.float64, device=dev)
        total_head = 0.0
        lines.append(f"  the head alone, level by level ({a.head_iters} calls back to back; bytes = 2 P h w c x 4, P = {hp}, one chunk):")
        for level, (f, lin) in enumerate(zip(taps, lins)):
            ts = [timed(lambda: ops.lpips_head(f, lin, net.eps, out=out, accumulate=level > 0), a.head_iters) for _ in range(a.rounds)]
            med, nbytes = statistics.median(ts), f.numel() * 4
            total_head += med
            where = "fits the Infinity Cache: re-read from there" if nbytes < 200 * 2 ** 20 else "larger than the Infinity Cache: from HBM"
            lines.append(f"    level {level} {tuple(f.shape)}: {med * 1e3:8.1f} us ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f})  {nbytes / 2 ** 20:7.1f} MiB  "
                         f"{nbytes / med / 1e9:7.3f} TB/s  ({where})")
        lines.append(f"    {len(taps)} levels: {total_head:.3f} ms = {100 * total_head * -(-p // net.chunk) / statistics.median(times['hip']):.1f} % of the hip call ({-(-p // net.chunk)} chunk(s))")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
