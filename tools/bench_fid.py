#!/usr/bin/env python
"""Times the two FID kernels (csrc/fid.hip) on one MI355X against the ATen / rocBLAS composition torchmetrics and evaluation/fid.py:61-64 run.

    python tools/bench_fid.py [--iters 20] [--rounds 5] [--out FILE]

  update_features   FID.update_features(X, real) at (N, F) = (32, 2048), (256, 2048), (1024, 2048), X f32 -- one dmvae_fid_accumulate launch and the sample
                    count's add -- against torchmetrics' update on the same states: `X.double()`, `sum += X.sum(0)`, `cov_sum += X.t().mm(X)`
  fid_resize_u8     32 x 3 x 256^2 -> 299^2, f32 and bf16, against `F.interpolate(mode="bicubic")`, `(x * 255).clamp(0, 255).to(torch.uint8)`

Rounds are interleaved: every round times every case on both routes, one after the other, so that a change of the machine's state hits both.  A time is the
mean over `--iters` calls between two device events after a warm-up call of the same shape; the table gives the median and the spread over the rounds, the
bytes the call has to move (accumulate: X in once -- its re-reads by every block of cov_sum are served by the caches and not counted --, the upper
triangle of cov_sum in, all of cov_sum out; resize: image in, uint8 out) and that traffic over the time as a fraction of the 8 TB/s HBM peak.  The 33.6 MB state of F = 2048 stays in the Infinity Cache
between back-to-back calls, so the fraction describes the loop as timed, not a cold call.  The f64 GEMM rate is 2 N F^2 / 2 FLOP (upper triangle) over the
time.  No CPU timing: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fid: needs a GPU (no CPU timing)")
    from dmvae_amd import ops
    from dmvae_amd.fid import FID

    class NoExtractor(torch.nn.Module):
        num_features = 2048

    g = torch.Generator(device="cuda").manual_seed(0)
    cases = []                                                  # (name, hip callable, stock callable, bytes moved, f64 flop or None)
    fid = FID(NoExtractor()).cuda()
    s2, c2, n2 = torch.zeros_like(fid.real_features_sum), torch.zeros_like(fid.real_features_cov_sum), torch.zeros_like(fid.real_features_num_samples)
    f = 2048
    for n in (32, 256, 1024):
        x = torch.randn(n, f, device="cuda", generator=g)

        def hip(x=x):
            fid.update_features(x, True)

        def stock(x=x):
            xd = x.double()
            s2.add_(xd.sum(dim=0))
            c2.add_(xd.t().mm(xd))
            n2.add_(x.shape[0])

        nbytes = n * f * 4 + (f * (f + 64) // 2) * 8 + f * f * 8 + 2 * f * 8
        cases.append((f"update_features N={n} F={f} f32", hip, stock, nbytes, n * f * (f + 64)))
    for dtype in (torch.float32, torch.bfloat16):
        img = torch.rand(32, 3, 256, 256, device="cuda", generator=g).to(dtype)

        def hip(img=img):
            ops.fid_resize_u8(img, 299)

        def stock(img=img):
            (F.interpolate(img, size=(299, 299), mode="bicubic") * 255).clamp(0, 255).to(dtype=torch.uint8)

        cases.append((f"fid_resize_u8 32x3x256^2->299^2 {str(dtype).split('.')[-1]}", hip, stock, img.numel() * img.element_size() + 32 * 3 * 299 * 299, None))

    times = {c[0]: ([], []) for c in cases}
    for _ in range(a.rounds):
        for name, hip, stock, _, _ in cases:
            times[name][0].append(timed(hip, a.iters))
            times[name][1].append(timed(stock, a.iters))
    lines = [f"tools/bench_fid.py --iters {a.iters} --rounds {a.rounds} on {torch.cuda.get_device_name(0)}: us per call, median [min .. max] over the rounds",
             f"{'case':48s} {'HIP kernel':>28s} {'ATen / rocBLAS':>28s} {'stock/HIP':>9s} {'MB moved':>9s} {'of 8 TB/s':>9s} {'f64 TFLOP/s':>11s}"]
    for name, _, _, nbytes, flop in cases:
        h, s = times[name]
        mh, ms = statistics.median(h), statistics.median(s)
        fmt = lambda v, m: f"{m:9.1f} [{min(v):7.1f} .. {max(v):7.1f}]"
        lines.append(f"{name:48s} {fmt(h, mh):>28s} {fmt(s, ms):>28s} {ms / mh:9.2f} {nbytes / 1e6:9.1f} {nbytes / (mh * 1e-6) / HBM_PEAK:9.3f} "
                     f"{(flop / (mh * 1e-6) / 1e12 if flop else float('nan')):11.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
