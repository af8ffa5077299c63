#!/usr/bin/env python
"""Times dmvae_amd.models.inception.InceptionV3Compat on one MI355X against the same module's stock f32 route, on the same device, in the same process.

    python tools/bench_inception.py [--batches 25,200] [--iters 3] [--rounds 3] [--out FILE]

  hip     `features_logits` on the kernels of csrc/inception.hip (exact f32 on v_mfma_f32_16x16x4_f32), normalised f32 [B, 3, 299, 299] in.
  stock   `forward_stock` of the same module with the same parameters: F.conv2d / F.batch_norm / F.relu / F.*_pool2d on f32 device tensors (the library's
          f32 convolutions).

Parameters are seeded random values (the published weights are not on this machine); times do not depend on them.  Rounds are interleaved: every round
times both routes, one after the other.  A time is the mean over `--iters` calls between two device events after a warm-up call of the same shape; the
table gives the median and the spread over the rounds.  The rate is the convolutions' 2 Ho Wo Cout Cin kh kw flops per image, recomputed from the module's
layer table (printed; the pools, the BatchNorm epilogues and the fc layer's 4.1 MFLOP are not counted), over the time: a whole-network rate in f32 TFLOP/s,
not a kernel's share of peak.  The per-stage share is taken in a separate pass with a device event after every stage of the table.  The largest relative
L2 distance between the two routes' features is printed too.  No CPU timing: without a GPU the tool fails."""
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


def conv_flops(net, size):
    """-> (flops per image of the 94 convolutions, {stage: flops}) by walking the layer table with the layers' own shape arithmetic."""
    from dmvae_amd.models.inception import LAYER_TABLE, BasicConv2d
    per_stage = {}

    def conv(m, hw):
        ho, wo = m.out_hw(*hw)
        return 2 * ho * wo * m.cout * m.cin * m.kernel[0] * m.kernel[1], (ho, wo)
    hw = (size, size)
    for name, make in LAYER_TABLE:
        fl = 0
        if make is None:
            hw = ((hw[0] - 3) // 2 + 1, (hw[1] - 3) // 2 + 1)
        else:
            m = getattr(net, name)
            if isinstance(m, BasicConv2d):
                fl, hw = conv(m, hw)
            else:
                out_hw = hw
                for branch in m.plan():
                    cur = hw
                    for step in branch:
                        if isinstance(step, str):
                            cur = ((cur[0] - 3) // 2 + 1, (cur[1] - 3) // 2 + 1) if step == "max2" else cur
                        else:
                            for s in (step if isinstance(step, tuple) else (step,)):
                                f, nxt = conv(s, cur)
                                fl += f
                            cur = nxt
                    out_hw = cur
                hw = out_hw
        per_stage[name] = fl
    return sum(per_stage.values()), per_stage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="25,200")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_inception: needs a GPU (no CPU timing)")
    from dmvae_amd.models.inception import InceptionV3Compat
    dev = "cuda:0"
    torch.manual_seed(0)
    net = InceptionV3Compat()
    with torch.no_grad():
        for _, m in net.conv_layers():                                 # eval-mode statistics that keep the activations alive
            m.bn.running_var.uniform_(0.5, 1.5)
            m.bn.running_mean.normal_(0, 0.1)
    net = net.to(dev)
    flops, per_stage = conv_flops(net, 299)
    lines = [f"InceptionV3Compat at 299 x 299: {flops / 2e9:.3f} GMAC = {flops / 1e9:.3f} GFLOP per image in the 94 convolutions (layer table)",
             f"device: {torch.cuda.get_device_name(0)}; iters {a.iters}, rounds {a.rounds}; times are medians over the rounds (min .. max)", ""]
    for b in (int(s) for s in a.batches.split(",")):
        x = torch.rand(b, 3, 299, 299, device=dev) * 2 - 1
        routes = {"hip": lambda: net.features_logits(x), "stock": lambda: net.forward_stock(x)}
        f_hip, f_stock = routes["hip"]()[0], routes["stock"]()[0]
        dist = ((f_hip.double() - f_stock.double()).norm(dim=1) / f_stock.double().norm(dim=1)).max().item()
        times = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, fn in routes.items():
                times[k].append(timed(fn, a.iters))
        lines.append(f"B = {b}   (largest per-image relative L2 distance between the routes' features: {dist:.2e})")
        for k, ts in times.items():
            med = statistics.median(ts)
            lines.append(f"  {k:6s} {med:9.2f} ms ({min(ts):.2f} .. {max(ts):.2f})   {b / med * 1e3:9.1f} images/s   {flops * b / med / 1e9:7.2f} TFLOP/s f32 (whole network)")
        lines.append(f"  hip / stock time: {statistics.median(times['hip']) / statistics.median(times['stock']):.2f}")
        # per-stage share: one instrumented pass (a chunk at most: the events of a second chunk would overwrite the first's)
        bs = min(b, net.chunk)
        xs = x[:bs].contiguous()
        events = []

        def hook(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append((name, e))
        net.features_logits(xs)
        torch.cuda.synchronize()
        start = torch.cuda.Event(enable_timing=True)
        net.stage_hook = hook
        net._operands(torch.device(dev))
        from dmvae_amd import ops
        xin = ops.inception_input(xs)
        feats, lo = torch.empty(bs, 2048, device=dev), torch.empty(bs, 1008, device=dev)
        start.record()
        net._hip_pass(xin, feats, lo, None)
        net.stage_hook = None
        torch.cuda.synchronize()
        total, prev = start.elapsed_time(events[-1][1]), start
        lines.append(f"  per-stage time of one pass of {bs} images ({total:.2f} ms up to the last stage; share of that, and the stage's conv TFLOP/s):")
        for name, e in events:
            ms = prev.elapsed_time(e)
            rate = f"{per_stage[name] * bs / ms / 1e9:6.2f} TFLOP/s" if per_stage[name] else "     (pool)"
            lines.append(f"    {name:14s} {ms:8.3f} ms  {100 * ms / total:5.1f} %  {rate}")
            prev = e
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
