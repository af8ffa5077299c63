#!/usr/bin/env python
"""Times the two kernels of csrc/fidelity.hip on one MI355X against the composed torch routes on the same device, in the same process.

    python tools/bench_fidelity.py [--iters 20] [--rounds 5] [--out FILE]

  resize     ops.resize_tf1_bilinear at B x 256 x 256 x 3 uint8 (NHWC, what `VAE.decode_uint8` hands over) -> B x 3 x 299 x 299 f32, B = 25 (one batch of
             sample_50k.py) and B = 1024: one launch.  Composed: permute + float, four index_select pairs, the two lerps along x, the lerp along y, the
             normalisation -- the form tests/test_fidelity_cpu.py holds the spec to, on f32 device tensors.
  IS         ops.inception_score at 50 000 x 1008 f32 logits, 10 splits, through a permutation table: three launches, f64.  Composed: the rows gathered
             through the same table, `softmax` / `log_softmax` on the f64 copy, and the loop over the splits (mean, log, KL, sum, mean, exp).

Rounds are interleaved: every round times every route, one after the other, so that a change of the machine's state hits all of them.  A time is the mean
over `--iters` calls between two device events after a warm-up call of the same shape; the table gives the median and the spread over the rounds.  Peak
memory is torch's allocator high-water mark over one call, above what was allocated before it (the inputs).  The bytes a kernel must move are counted from
the shape (resize: the uint8 input once, the f32 output once; IS: the logits twice -- the row pass re-reads its row from cache, the marginal pass reads it
again) and the rate printed is that count over the time, not a share of any peak.  `ops.inception_score`'s time includes its range check of the table (one
reduction and one synchronisation).  The largest difference between the two routes' values is printed as well.  No CPU timing: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys

import numpy as np
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
    return e0.elapsed_time(e1) * 1e3 / iters                    # us per call


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def composed_resize(u8_nhwc, size):
    x = u8_nhwc.permute(0, 3, 1, 2).float()
    h, w = x.shape[-2:]

    def taps(n_in):
        g = torch.arange(size, dtype=torch.float32, device=x.device) * (n_in / size)
        i0 = g.floor().long()
        return i0, (i0 + 1).clamp(max=n_in - 1), g - i0.float()
    y0, y1, dy = taps(h)
    x0, x1, dx = taps(w)
    dy, dx = dy.view(1, 1, size, 1), dx.view(1, 1, 1, size)
    r0, r1 = x.index_select(2, y0), x.index_select(2, y1)
    a, b, c, d = r0.index_select(3, x0), r0.index_select(3, x1), r1.index_select(3, x0), r1.index_select(3, x1)
    top = a + (b - a) * dx
    bot = c + (d - c) * dx
    return ((top + (bot - top) * dy) - 128) / 128


def composed_isc(logits, order, splits):
    x = logits[order].double()
    p, logp = x.softmax(dim=1), x.log_softmax(dim=1)
    n, out = x.shape[0], []
    for k in range(splits):
        pk, lk = p[k * n // splits:(k + 1) * n // splits], logp[k * n // splits:(k + 1) * n // splits]
        out.append((pk * (lk - pk.mean(dim=0, keepdim=True).log())).sum(dim=1).mean().exp())
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fidelity: needs a GPU (no CPU timing)")
    from dmvae_amd import ops

    g = torch.Generator(device="cuda").manual_seed(0)
    small = torch.randint(0, 256, (25, 256, 256, 3), dtype=torch.uint8, device="cuda", generator=g)
    large = torch.randint(0, 256, (1024, 256, 256, 3), dtype=torch.uint8, device="cuda", generator=g)
    n, classes, splits = 50000, 1008, 10
    logits = torch.randn(n, classes, device="cuda", generator=g) * 4
    order = torch.from_numpy(np.random.RandomState(0).permutation(n)).cuda()

    def moved_resize(u8):
        return u8.numel() + u8.shape[0] * 3 * 299 * 299 * 4
    groups = [
        ("resize 25 x 256 x 256 -> 299", moved_resize(small), [("kernel", lambda: ops.resize_tf1_bilinear(small, 299)), ("composed torch f32", lambda: composed_resize(small, 299))]),
        ("resize 1024 x 256 x 256 -> 299", moved_resize(large), [("kernel", lambda: ops.resize_tf1_bilinear(large, 299)), ("composed torch f32", lambda: composed_resize(large, 299))]),
        (f"IS {n} x {classes}, {splits} splits", 2 * logits.numel() * 4, [("kernel f64", lambda: ops.inception_score(logits, order, splits)),
                                                                          ("composed torch f64", lambda: composed_isc(logits, order, splits))]),
    ]
    times = {(gn, rn): [] for gn, _, routes in groups for rn, _ in routes}
    for _ in range(a.rounds):
        for gn, _, routes in groups:
            for rn, fn in routes:
                times[(gn, rn)].append(timed(fn, a.iters))
    lines = [f"tools/bench_fidelity.py --iters {a.iters} --rounds {a.rounds} on {torch.cuda.get_device_name(0)}: us per call, median [min .. max] over the rounds",
             f"{'route':52s} {'us per call':>34s} {'composed/this':>13s} {'peak MB':>9s} {'GB/s':>7s}"]
    for gn, moved, routes in groups:
        base = statistics.median(times[(gn, routes[1][0])])
        for rn, fn in routes:
            v = times[(gn, rn)]
            m = statistics.median(v)
            rate = f"{moved / (m * 1e-6) / 1e9:7.0f}" if rn.startswith("kernel") else f"{'-':>7s}"
            lines.append(f"{gn + ': ' + rn:52s} {m:12.1f} [{min(v):9.1f} .. {max(v):9.1f}] {base / m:13.2f} {peak_bytes(fn) / 1e6:9.2f} {rate}")
    d_resize = (ops.resize_tf1_bilinear(small, 299) - composed_resize(small, 299)).abs().max().item()
    k, c = ops.inception_score(logits, order, splits), composed_isc(logits, order, splits)
    lines.append(f"max |kernel - composed|: resize {d_resize:.1e}; IS relative {((k - c).abs() / c).max().item():.2e} (scores {c.min().item():.4f} .. {c.max().item():.4f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
