#!/usr/bin/env python
"""Times the SSIM kernel (csrc/ssim.hip) on one MI355X against the composed torch route in f32 on the same device, in the same process.

    python tools/bench_ssim.py [--iters 50] [--rounds 5] [--batch 32] [--size 256] [--out FILE]

  kernel     ops.ssim(a, b) at B x 3 x S x S, f32 and bf16: two launches (tiles, finalize), window moments in f64
  composed   the algorithm torchmetrics runs, restated literally in f32: reflect-pad both images by 5, concatenate p, t, p p, t t, p t (5 B images),
             one depthwise 11 x 11 conv2d, the moments, the SSIM map, crop 5 from every side, per-image mean

Rounds are interleaved: every round times every route, one after the other, so that a change of the machine's state hits all of them.  A time is the mean
over `--iters` calls between two device events after a warm-up call of the same shape; the table gives the median and the spread over the rounds.  Peak
memory is torch's allocator high-water mark over one call, above what was allocated before it (the inputs).  The f64 work the kernel does is counted from
the shape, per 32 x 16 output tile: the horizontal pass forms 3 products for each of the 14 pixels under four adjacent windows and 4 x 11 x 5 multiply-adds,
for 26 halo rows x 8 column groups; the vertical pass 11 x 5 multiply-adds per output pixel.  The rate printed is that count over the time, not a share of
any peak.  The difference between the two routes' values is printed as well: it is the f32 route's error (tests/test_gpu_ssim.py holds the kernel to 1e-9
of an f64 witness).  No CPU timing: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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
    return e0.elapsed_time(e1) * 1e3 / iters                    # us per call


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def composed_f32(p, t, kernel, c1=0.01 ** 2, c2=0.03 ** 2):
    b, c = p.shape[:2]
    p, t = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    out = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), kernel, groups=c).split(b)
    mpp, mtt, mpt = out[0].pow(2), out[1].pow(2), out[0] * out[1]
    sp, st, spt = torch.clamp(out[2] - mpp, min=0.0), torch.clamp(out[3] - mtt, min=0.0), out[4] - mpt
    full = ((2 * mpt + c1) * (2 * spt + c2)) / ((mpp + mtt + c1) * (sp + st + c2))
    return full[..., 5:-5, 5:-5].reshape(b, -1).mean(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim: needs a GPU (no CPU timing)")
    from dmvae_amd import ops

    b, c, s = a.batch, 3, a.size
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(b, c, s, s, device="cuda", generator=g)
    y = (x + 0.02 * torch.randn(b, c, s, s, device="cuda", generator=g)).clamp(0, 1)
    xb, yb = x.bfloat16(), y.bfloat16()
    d = torch.arange(11, device="cuda", dtype=torch.float32) - 5
    w1 = torch.exp(-(d / 1.5) ** 2 / 2)
    w1 = (w1 / w1.sum()).unsqueeze(0)
    kernel = torch.matmul(w1.t(), w1).expand(c, 1, 11, 11).contiguous()

    routes = [("kernel f32 in, f64 moments", lambda: ops.ssim(x, y)), ("kernel bf16 in, f64 moments", lambda: ops.ssim(xb, yb)),
              ("composed torch f32", lambda: composed_f32(x, y, kernel))]
    times = {n: [] for n, _ in routes}
    for _ in range(a.rounds):
        for n, fn in routes:
            times[n].append(timed(fn, a.iters))
    peaks = {n: peak_bytes(fn) for n, fn in routes}
    diff = (ops.ssim(x, y) - composed_f32(x, y, kernel).double()).abs().max().item()

    outs = (s - 10) * (s - 10)
    tiles = -(-(s - 10) // 32) * -(-(s - 10) // 16)
    fma = b * c * tiles * (26 * 8 * (14 * 3 + 4 * 11 * 5) + 16 * 32 * 11 * 5)    # horizontal pass (halo rows included) + vertical pass, per tile
    base = statistics.median(times["composed torch f32"])
    lines = [f"tools/bench_ssim.py --iters {a.iters} --rounds {a.rounds} on {torch.cuda.get_device_name(0)}: {b} x {c} x {s} x {s}, us per call, "
             f"median [min .. max] over the rounds",
             f"{'route':32s} {'us per call':>30s} {'composed/this':>13s} {'peak MB':>9s} {'f64 Gop/s':>10s}"]
    for n, _ in routes:
        v = times[n]
        m = statistics.median(v)
        rate = f"{fma / (m * 1e-6) / 1e9:10.0f}" if n.startswith("kernel") else f"{'-':>10s}"
        lines.append(f"{n:32s} {m:10.1f} [{min(v):8.1f} .. {max(v):8.1f}] {base / m:13.2f} {peaks[n] / 1e6:9.2f} {rate}")
    lines.append(f"inputs: {2 * x.numel() * 4 / 1e6:.1f} MB (f32), {2 * x.numel() * 2 / 1e6:.1f} MB (bf16); {b * c * outs} output pixels; "
                 f"max |kernel - composed f32| per image {diff:.2e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
