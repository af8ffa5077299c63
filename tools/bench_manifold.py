#!/usr/bin/env python
"""Times the kernels of csrc/manifold.hip on one MI355X against the composition torch-fidelity uses, on the same device, in the same process.

    python tools/bench_manifold.py [--sizes 10000,50000] [--features 2048] [--iters 2] [--rounds 3] [--out FILE]

  knn_radius   ops.knn_radius at N x F f32, k = 3.  Composed: torch-fidelity's loop -- row batches of 10 000, `torch.cdist` against column parts of 10 000
               concatenated to [10 000, N], `kthvalue(k + 1)` -- on f32 device tensors, WITHOUT the library's copies of every part to the host.
  member       ops.manifold_member of N queries against N references.  Composed: the same cdist loop, `(dist <= radii).any(dim=1)`.
  prc          both radii and both memberships: what `FidelityMetrics.compute(prc=True)` launches.  Composed: the same four loops.
  kid          ops.kid_mmd2 at 100 subsets of 1000 rows out of N (tables from `fidelity.kid_subset_tables`).  Composed: per subset the three f64 kernel
               matrices of the gathered rows (the library does this in numpy on the host; here torch f64 on the device).

Rounds are interleaved: every round times every route, one after the other.  A time is the mean over `--iters` calls between two device events after a
warm-up call of the same shape; the table gives the median and the spread over the rounds.  The rate is the Gram's 2 N M F flops (KID: three Grams of 2 m m F
per subset) over the time, in f64 TFLOP/s for the kernels -- the selection, comparison and polynomial epilogues are not counted.  Peak memory is torch's
allocator high-water mark over one call, above what was allocated before it (the inputs).  The largest difference between the two routes' values is printed
too: the composed distances are f32 square roots, the kernels' f64 squares, so radii differ at f32 accuracy and memberships may differ for queries within
that of a surface.  No CPU timing: without a GPU the tool fails."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PART = 10000


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


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def cdist_part(a, b):
    return torch.cat([torch.cdist(a, part) for part in b.split(PART)], dim=1)


def composed_radii(x, k):
    return torch.cat([cdist_part(batch, x).kthvalue(k + 1).values for batch in x.split(PART)])


def composed_member(q, r, radii):
    return torch.cat([(cdist_part(batch, r) <= radii).any(dim=1) for batch in q.split(PART)])


def composed_prc(fake, real, k):
    return composed_member(fake, real, composed_radii(real, k)).float().mean(), composed_member(real, fake, composed_radii(fake, k)).float().mean()


def composed_kid(x, y, idx1, idx2, degree=3, coef0=1.0):
    gamma, out = 1.0 / x.shape[1], []
    for i1, i2 in zip(idx1, idx2):
        a, b = x[i1].double(), y[i2].double()
        m = a.shape[0]
        kxx, kyy, kxy = ((gamma * u.mm(v.t()) + coef0) ** degree for u, v in ((a, a), (b, b), (a, b)))
        out.append((kxx.sum() - kxx.diagonal().sum() + kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1)) - 2 * kxy.sum() / (m * m))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,50000")
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_manifold: needs a GPU (no CPU timing)")
    from dmvae_amd import fidelity, ops

    f, k, subsets, m = a.features, 3, 100, 1000
    prop = torch.cuda.get_device_properties(0)
    lines = [f"tools/bench_manifold.py --sizes {a.sizes} --features {f} --iters {a.iters} --rounds {a.rounds} on one {torch.cuda.get_device_name(0)} "
             f"({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB): ms per call, median [min .. max] over the rounds",
             f"{'route':58s} {'ms per call':>34s} {'composed/this':>13s} {'peak MB':>10s} {'TFLOP/s':>8s}"]
    for n in (int(s) for s in a.sizes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(n)
        fake = torch.randn(n, f, device="cuda", generator=g).abs_()                   # pooled post-ReLU features are non-negative
        real = (torch.randn(n, f, device="cuda", generator=g) * 1.05).abs_()
        rad = ops.knn_radius(real, k)
        rad_c = composed_radii(real, k)
        t1, t2 = (torch.from_numpy(t).cuda() for t in fidelity.kid_subset_tables(n, n, subsets, m, 0))

        def prc_kernels():
            return (ops.manifold_member(fake, real, ops.knn_radius(real, k)).float().mean(), ops.manifold_member(real, fake, ops.knn_radius(fake, k)).float().mean())
        gram = 2.0 * n * n * f
        groups = [
            (f"knn_radius {n} x {f}, k = {k}", gram, [("kernels f64", lambda: ops.knn_radius(real, k)), ("composed cdist f32 + kthvalue", lambda: composed_radii(real, k))]),
            (f"member {n} in {n} x {f}", gram, [("kernels f64", lambda: ops.manifold_member(fake, real, rad)), ("composed cdist f32 + any", lambda: composed_member(fake, real, rad_c))]),
            (f"prc {n} / {n} x {f}", 4 * gram, [("kernels f64", prc_kernels), ("composed", lambda: composed_prc(fake, real, k))]),
            (f"kid {subsets} x {m} of {n} x {f}", 3 * subsets * 2.0 * m * m * f, [("kernels f64", lambda: ops.kid_mmd2(fake, real, t1, t2)),
                                                                                  ("composed torch f64", lambda: composed_kid(fake, real, t1, t2))]),
        ]
        times = {(gn, rn): [] for gn, _, routes in groups for rn, _ in routes}
        for _ in range(a.rounds):
            for gn, _, routes in groups:
                for rn, fn in routes:
                    times[(gn, rn)].append(timed(fn, a.iters))
        for gn, flops, routes in groups:
            base = statistics.median(times[(gn, routes[1][0])])
            for rn, fn in routes:
                v = times[(gn, rn)]
                med = statistics.median(v)
                rate = f"{flops / (med * 1e-3) / 1e12:8.2f}" if rn.startswith("kernels") else f"{'-':>8s}"
                lines.append(f"{gn + ': ' + rn:58s} {med:12.2f} [{min(v):9.2f} .. {max(v):9.2f}] {base / med:13.2f} {peak_bytes(fn) / 1e6:10.1f} {rate}")
        d_rad = ((rad.sqrt() - rad_c.double()).abs() / rad_c.double()).max().item()
        mk, mc = ops.manifold_member(fake, real, rad), composed_member(fake, real, rad_c)
        kk, kc = ops.kid_mmd2(fake, real, t1, t2), composed_kid(fake, real, t1, t2)
        pk, pc = prc_kernels(), composed_prc(fake, real, k)
        lines.append(f"N = {n}: max relative |sqrt(radius2) - composed radius| {d_rad:.2e}; memberships that differ {int((mk.bool() != mc).sum().item())} of {n}; "
                     f"precision / recall kernels {pk[0].item():.4f} / {pk[1].item():.4f}, composed {pc[0].item():.4f} / {pc[1].item():.4f}; "
                     f"KID max |kernels - composed| {(kk - kc).abs().max().item():.2e} (mean {kc.mean().item():.4e})")
        del fake, real, rad, rad_c
        torch.cuda.empty_cache()
    lines += ["notes (printed by the tool): no clock is read, set or pinned.  Times are between device events and include, for the kernels, the workspace allocation of",
              "each call and (kid) ops.kid_mmd2's range check of the two tables (torch.aminmax + one synchronisation); for the composition, f32 torch.cdist in",
              f"{PART}-column parts + kthvalue / any on the device, without torch-fidelity's copies of every part to the host.  TFLOP/s: the Grams' 2 N M F flops (kid:",
              "3 x 100 Grams of 2 m m F) over the time, in f64; the MI355X's f64 matrix peak is 78.6 TFLOP/s.  Peak MB: the allocator's high-water mark above the inputs."]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
