#!/usr/bin/env python
"""Times the device-side input pipeline (dmvae_amd/data.py, csrc/data.hip) on one MI355X, and beside it the pipeline it replaces -- PIL's `train_aug`
(utils/build_dataset.py:55-66) -- on the same box's CPUs.

    python tools/bench_data.py [--window 0.3] [--rounds 5] [--out FILE]

Batches (image_size 256, mid_reso 1.5, train mode with flips, seeded draws):
  uniform   B = 32 of 500 x 375 (W x H)
  mixed     B = 32 of ImageNet-like sizes, 160 x 120 up to 3000 x 2000

Per batch and round, one after the other so that a change of the machine's state hits every row:
  kernel        dmvae_image_preprocess alone (tables already on the device), f32 NCHW and u8 NHWC output: mean over a window of back-to-back launches
                between two device events, as many launches as fill --window seconds (counted from a short trial), after a warm-up launch.  The same pack
                is read by every launch of a window, so an 18 MB pack is served from L2 / the Infinity Cache: a warm-cache time, not a cold call
  H2D pack      the pinned pack's copy to the device, same timing
  tables cold   DeviceInputPipeline.tables on the host with the table cache emptied before every call (the Lanczos coefficients of the crop window, two
                axes per image; what a train-mode batch of random crops pays): host clock, per batch
  tables hit    the same call again: every axis comes from the cache (what a val-mode batch of sizes seen before pays)
  apply         draw + tables + their upload + launch in train mode (fresh random crops every call, so the cache rarely hits), host clock around a device
                synchronise: what a training loop pays per batch when nothing overlaps
  PIL 1 / 16    flip, Image.resize(LANCZOS), crop, float conversion per image with PIL and numpy on 1 thread and on 16 threads (PIL releases the GIL in
                its resampler; the reference uses worker processes, which this does not reproduce), host clock; torchvision is not needed

"MB" is what the kernel has to move at least (the decoded images in once, the batch out); the fraction of the 8 TB/s HBM peak is that over the kernel time,
a lower bound of the traffic, not a counter reading.  Without a GPU the tool fails; without PIL the PIL rows say so."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_PEAK = 8.0e12
MIXED = [(500, 375), (375, 500), (500, 333), (333, 500), (640, 480), (480, 640), (1024, 768), (800, 600), (1600, 1200), (256, 256), (160, 120), (500, 500),
         (3000, 2000), (2048, 1536), (400, 300), (500, 374)]               # (W, H), cycled to B


def _event_window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def event_us(fn, window):
    fn()
    torch.cuda.synchronize()
    trial = _event_window(fn, 20)
    return _event_window(fn, max(50, int(window * 1e6 / trial)))


def _host_window(fn, iters):
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / iters


def host_us(fn, window):
    fn()
    torch.cuda.synchronize()
    trial = _host_window(fn, 3)
    return _host_window(fn, max(5, int(window * 1e6 / trial)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_data: needs a GPU (no CPU timing of the kernel)")
    from dmvae_amd import data as D
    from dmvae_amd import ops
    from dmvae_amd.data import DeviceInputPipeline, pack_images, resized_size
    try:
        from PIL import Image
    except ImportError:
        Image = None

    rng = np.random.default_rng(0)
    batches = {"uniform 32 x (500 x 375)": [(500, 375)] * a.batch, "mixed ImageNet-like": [MIXED[i % len(MIXED)] for i in range(a.batch)]}
    S, MID = 256, 384
    rows, cases = [], []
    for name, sizes in batches.items():
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
        pipe = DeviceInputPipeline(S, 1.5, "train", True, generator=torch.Generator().manual_seed(1))
        ragged = pack_images(imgs)
        dev = ragged.to("cuda")
        flip, top, left = pipe.draw(ragged)
        rec, taps = pipe.tables(ragged, flip, top, left)
        rec_d, taps_d = rec.cuda(), taps.cuda()
        out_f = torch.empty(len(imgs), 3, S, S, device="cuda")
        out_u = torch.empty(len(imgs), S, S, 3, dtype=torch.uint8, device="cuda")
        pil = [Image.fromarray(x) for x in imgs] if Image is not None else None

        def pil_one(i, pil=pil, flip=flip, top=top, left=left):
            im = pil[i]
            if flip[i]:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            ow, oh = resized_size(im.size[0], im.size[1], MID)
            if (ow, oh) != im.size:
                im = im.resize((ow, oh), Image.LANCZOS)
            l, t = int(left[i]), int(top[i])
            x = np.asarray(im.crop((l, t, l + S, t + S))).transpose(2, 0, 1).astype(np.float32) / np.float32(255)      # numpy: no intra-op thread pool
            return (x + x) + np.float32(-1)

        def pil_batch(pool, n=len(imgs), one=pil_one):
            return torch.from_numpy(np.stack(list(pool.map(one, range(n))) if pool else [one(i) for i in range(n)]))

        def fns_of(dev=dev, rec_d=rec_d, taps_d=taps_d, out_f=out_f, out_u=out_u, ragged=ragged, pipe=pipe, flip=flip, top=top, left=left):
            return {
                "kernel f32": (event_us, lambda: ops.image_preprocess(dev.data, rec_d, taps_d, S, "f32", out_f)),
                "kernel u8": (event_us, lambda: ops.image_preprocess(dev.data, rec_d, taps_d, S, "u8", out_u)),
                "H2D pack": (event_us, lambda: ragged.to("cuda", non_blocking=True)),
                "tables cold": (host_us, lambda: (D._axis_table.cache_clear(), pipe.tables(ragged, flip, top, left))),
                "tables hit": (host_us, lambda: pipe.tables(ragged, flip, top, left)),
                "apply f32": (host_us, lambda: pipe(dev)),
            }

        fns = fns_of()
        nbytes = {"kernel f32": ragged.data.numel() + out_f.numel() * 4, "kernel u8": ragged.data.numel() + out_u.numel(), "H2D pack": ragged.data.numel()}
        cases.append((name, len(imgs), fns, nbytes, pil_batch if pil else None))
    times = {}
    pool16 = ThreadPoolExecutor(16)
    for _ in range(a.rounds):
        for name, n, fns, _, pil_batch in cases:
            for k, (timer, fn) in fns.items():
                times.setdefault((name, k), []).append(timer(fn, a.window))
            if pil_batch:
                for k, pool in (("PIL 1 thread", None), ("PIL 16 threads", pool16)):
                    t = time.perf_counter()
                    pil_batch(pool)
                    times.setdefault((name, k), []).append((time.perf_counter() - t) * 1e6)
    pool16.shutdown()
    lines = [f"tools/bench_data.py --window {a.window} --rounds {a.rounds} --batch {a.batch} on {torch.cuda.get_device_name(0)}, {os.cpu_count()} CPUs visible, "
             f"{len(os.sched_getaffinity(0))} usable; image_size 256, mid 384, train mode",
             "us per batch, median [min .. max] over the rounds; per image = median / B",
             f"{'batch':28s} {'row':16s} {'us per batch':>34s} {'us / image':>11s} {'images/s':>11s} {'MB':>7s} {'of 8 TB/s':>9s}"]
    for name, n, fns, nbytes, pil_batch in cases:
        keys = list(fns) + (["PIL 1 thread", "PIL 16 threads"] if pil_batch else [])
        for k in keys:
            v = times[(name, k)]
            m = statistics.median(v)
            nb = nbytes.get(k)
            lines.append(f"{name:28s} {k:16s} {m:12.1f} [{min(v):9.1f} .. {max(v):9.1f}] {m / n:11.2f} {n / (m * 1e-6):11.0f} "
                         + (f"{nb / 1e6:7.1f} {nb / (m * 1e-6) / HBM_PEAK:9.3f}" if nb and k != "H2D pack" else (f"{nb / 1e6:7.1f} {'':>9s}" if nb else "")))
        if not pil_batch:
            lines.append(f"{name:28s} PIL rows: PIL is not installed on this box, not measured")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
