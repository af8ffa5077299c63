"""Attention kernels at the shapes of the DMD / diffusion stages: LightningDiT-XL/1 heads (16 x 72 channels, 256 tokens, q / k padded to 96) at B = 16 / 64 and
ViT-L/16's packed qkv (16 x 64, 257 tokens) at B = 16 / 32: forward (+ row statistics) and the backward on those statistics, us per call and the algorithmic
bytes (every operand once, every result once) over that time.

Streaming section (`--stream-only` runs it alone, `--out FILE` also writes its table to FILE): the encoder's attention beyond the resident kernel's 288 tokens
(csrc/attention_stream.hip) at S = 577 and 1025, B x H = 32 x 16, random data, against the same attention composed from this build's own ops (f32-score GEMM +
row softmax + GEMM on head-major copies, keys padded to a multiple of 32 and masked) and the resident kernel at S = 288 for scale; rounds interleaved in one
process, median and minimum; 4 S^2 64 FLOP per head.  Then the frozen ViT-L forward at 1025 tokens (patch 8 at 256 px), B = 8: the HIP route against the stock
modules under autocast(bf16) -- the only way to run that shape before the streaming kernel.

`--stream-bwd` runs the backward section alone (`--out FILE` writes its table): `ops.attention_bwd_qkv_stream` (csrc/attention_bwd_stream.hip) against the
GEMM-composed `functional._attention_bwd` at S = 577 and 1025, B x H = 32 x 16, rounds interleaved in one process, median and minimum; 10 S^2 64 FLOP per head
(the five products of the minimal form; the kernels run seven).  Then the peak allocation of one trainable ViT-L block's backward at 1025 tokens, B = 16, on
either attention backward.

`--heads-stream` / `--heads-stream-bwd` (either or both in one run; `--out FILE` writes their tables): LightningDiT's attention beyond 288 tokens on head-major
operands -- `ops.attention_heads_stream` / `ops.attention_bwd_heads_stream` (the same two source files, instantiated at the staged head dims 64 and 96) against the
composed route of `lightningdit_fast._attention` / `functional.DitBlockFn` built from this build's own ops (f32-score GEMM + row softmax + GEMM, P saved for the
backward), at B x H = 16 x 16, N = 576 and 1024, D = 72 and 64; rounds interleaved in one process, median, minimum and spread.

`--wide` (`--out FILE` writes its table): the decoder AttnBlock's one head of 512 channels -- `ops.attention_wide_stream` (csrc/attention_wide.hip) against the
composed forward of `functional.AttnBlockFn` (gemm_nt + softmax_rows + transpose_last2 + gemm_nt) at B = 32, S = 2304 (384 px), 4096 (512 px) and 1024 (the 256-px
training shape, which stays on the composed route), rounds interleaved in one process; 4 S^2 512 FLOP per sample.  Then the allocation of one AttnBlock(512)
forward + backward at S = 4096, B = 8, on either route: what the forward leaves allocated, and the peak of forward + backward.

`--wide-bwd` (`--out FILE` writes its table): that attention's backward -- `ops.attention_wide_bwd_stream` (csrc/attention_wide_bwd.hip) against the backward
`functional.AttnBlockFn` ran above 1024 tokens before it (P recomputed by gemm_nt + softmax_rows, then gemm_nt + softmax_rows_bwd + gemm_tn + gemm_nt + gemm_tn) at
B = 32, S = 1024, 2304 and 4096, rounds interleaved in one process; 10 S^2 512 FLOP per sample (the five products of the minimal form; the kernels run eleven -- S and dP three times, the two dS products
twice each as hi + lo, P^T dO once -- the recomputing route six).  Then the allocation table of `--wide` again with the streaming backward in it."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dmvae_amd import ops

BF = torch.bfloat16


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


g = torch.Generator(device="cuda").manual_seed(0)
SECTION_ONLY = any(f in sys.argv for f in ("--stream-only", "--stream-bwd", "--heads-stream", "--heads-stream-bwd", "--wide", "--wide-bwd"))
for B in (() if SECTION_ONLY else (16, 32, 64)):
    H, N, D, DP = 16, 256, 72, 96
    q = torch.zeros(B * H, N, DP, device="cuda", dtype=BF); k = torch.zeros_like(q)
    q[..., :D] = torch.randn(B * H, N, D, device="cuda", generator=g).to(BF); k[..., :D] = torch.randn(B * H, N, D, device="cuda", generator=g).to(BF)
    v = torch.randn(B * H, N, D, device="cuda", generator=g).to(BF)
    scale = D ** -0.5
    out, lse = ops.attention_heads(q, k, v, B, scale, need_lse=True)
    dout = torch.randn(out.shape, device="cuda", generator=g).to(BF)
    tf = timed(lambda: ops.attention_heads(q, k, v, B, scale, need_lse=True))
    tb = timed(lambda: ops.attention_bwd_heads(q, k, v, out, dout, B, scale, lse=lse))
    fb = (2 * q.numel() + v.numel() + out.numel()) * 2 + lse.numel() * 4
    bb = (4 * q.numel() + 2 * v.numel() + 2 * out.numel()) * 2 + lse.numel() * 4
    fl = 4 * B * H * N * N * D
    print(f"DiT heads B={B:3d}: fwd+lse {tf:6.1f} us ({fb / tf * 1e-6:5.2f} TB/s, {fl / tf * 1e-6:5.0f} TF/s)   bwd lse {tb:6.1f} us ({bb / tb * 1e-6:5.2f} TB/s, {2.5 * fl / tb * 1e-6:5.0f} TF/s)")
for B in (() if SECTION_ONLY else (16, 32)):
    H, N, D = 16, 257, 64
    qkv = torch.randn(B, N, 3 * H * D, device="cuda", generator=g).to(BF)
    scale = D ** -0.5
    out, lse = ops.attention_qkv(qkv, H, scale, need_lse=True)
    dout = torch.randn(out.shape, device="cuda", generator=g).to(BF)
    tf = timed(lambda: ops.attention_qkv(qkv, H, scale, need_lse=True))
    tb = timed(lambda: ops.attention_bwd_qkv(qkv, out, dout, H, scale, lse=lse))
    fb = (qkv.numel() + out.numel()) * 2 + lse.numel() * 4
    bb = (2 * qkv.numel() + 2 * out.numel()) * 2 + lse.numel() * 4
    fl = 4 * B * H * N * N * D
    print(f"ViT qkv   B={B:3d}: fwd+lse {tf:6.1f} us ({fb / tf * 1e-6:5.2f} TB/s, {fl / tf * 1e-6:5.0f} TF/s)   bwd lse {tb:6.1f} us ({bb / tb * 1e-6:5.2f} TB/s, {2.5 * fl / tb * 1e-6:5.0f} TF/s)")


# ---- streaming kernel beyond 288 tokens ------------------------------------------------------------------------------------------------------------------
def composed(q, k, v, s, scale):
    """q, k, v: head-major [B*H, sp, 64] bf16 (rows >= s zero) -> [B*H, sp, 64]: what `functional._attention_bwd` / `lightningdit_fast._attention` compose"""
    sc = ops.gemm_nt(q, k, out_f32=True)
    if sc.shape[-1] != s:
        sc[:, :, s:] = float("-inf")
    return ops.gemm_nt(ops.softmax_rows(sc, scale), ops.transpose_last2(v))


def stream_section(out_path):
    B, H, D, scale = 32, 16, 64, 64 ** -0.5
    cases = {}
    for S in (288, 577, 1025):
        qkv = torch.randn(B, S, 3 * H * D, device="cuda", generator=g).to(BF)
        if S <= 288:
            cases[f"resident kernel      S={S:4d}"] = (S, lambda qkv=qkv: ops.attention_qkv(qkv, H, scale, need_lse=True))
            cases[f"streaming kernel     S={S:4d}"] = (S, lambda qkv=qkv: ops.attention_qkv_stream(qkv, H, scale, need_lse=True))
            continue
        sp = (S + 31) // 32 * 32
        hm = torch.zeros(3, B * H, sp, D, device="cuda", dtype=BF)
        hm[:, :, :S] = qkv.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).reshape(3, B * H, S, D)
        a = ops.attention_qkv_stream(qkv, H, scale).view(B, S, H, D).permute(0, 2, 1, 3).reshape(B * H, S, D).float()
        c = composed(hm[0], hm[1], hm[2], S, scale)[:, :S].float()
        print(f"S={S}: streaming vs composed rel-L2 {((a - c).norm() / c.norm()).item():.2e}")
        cases[f"streaming kernel     S={S:4d}"] = (S, lambda qkv=qkv: ops.attention_qkv_stream(qkv, H, scale, need_lse=True))
        cases[f"streaming, no lse    S={S:4d}"] = (S, lambda qkv=qkv: ops.attention_qkv_stream(qkv, H, scale))
        cases[f"composed (own ops)   S={S:4d}"] = (S, lambda hm=hm, S=S: composed(hm[0], hm[1], hm[2], S, scale))
    times = {k: [] for k in cases}
    for _ in range(7):                      # interleaved rounds
        for k, (S, fn) in cases.items():
            times[k].append(timed(fn, n=20))
    lines = [f"attention forward, B x H = {B} x {H}, head dim 64, random data, 7 interleaved rounds of 20 calls; TFLOP/s on 4 S^2 64 FLOP per head",
             f"{'case':32s} {'median us':>10s} {'min us':>10s} {'TF/s (median)':>14s} {'TF/s (min)':>11s}"]
    for k, (S, _) in cases.items():
        t = sorted(times[k])
        med, mn, fl = t[len(t) // 2], t[0], 4.0 * B * H * S * S * D
        lines.append(f"{k:32s} {med:10.1f} {mn:10.1f} {fl / med * 1e-6:14.1f} {fl / mn * 1e-6:11.1f}")
    # frozen ViT-L forward at 1025 tokens
    from dmvae_amd.models.vit import DinoV2ViT
    torch.manual_seed(0)
    vit = DinoV2ViT(embed_dim=1024, depth=24, num_heads=16, patch_size=8, img_size=256).cuda().eval()
    img = torch.randn(8, 3, 256, 256, device="cuda", generator=g)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        routes = {"HIP route (streaming attention)": lambda: vit.forward_features(img), "stock modules (autocast bf16)": lambda: vit.forward_features_stock(img)}
        y0, y1 = (f().float() for f in routes.values())
        vt = {k: [] for k in routes}
        for _ in range(5):
            for k, fn in routes.items():
                vt[k].append(timed(fn, n=5) * 1e-3)
    lines.append("")
    lines.append(f"frozen ViT-L/8 forward at 256 px (1025 tokens), B = 8, ms per call, 5 interleaved rounds of 5 calls; HIP vs stock relative norm {((y0 - y1).norm() / y1.norm()).item():.2e}")
    for k in routes:
        t = sorted(vt[k])
        lines.append(f"{k:32s} median {t[len(t) // 2]:8.2f} ms   min {t[0]:8.2f} ms")
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


# ---- streaming backward beyond 288 tokens ------------------------------------------------------------------------------------------------------------------
def stream_bwd_section(out_path):
    from dmvae_amd import functional as Fn
    B, H, D, scale = 32, 16, 64, 64 ** -0.5
    cases = {}
    lines = []
    for S in (577, 1025):
        qkv = torch.randn(B, S, 3 * H * D, device="cuda", generator=g).to(BF)
        out, lse = ops.attention_qkv_stream(qkv, H, scale, need_lse=True)
        dout = torch.randn(out.shape, device="cuda", generator=g).to(BF)
        a, c = ops.attention_bwd_qkv_stream(qkv, out, dout, H, scale, lse).float(), Fn._attention_bwd(qkv, dout, H, scale).float()
        lines.append(f"S={S}: streaming vs composed d(qkv) rel-L2 {((a - c).norm() / c.norm()).item():.2e}")
        del a, c
        cases[f"streaming kernels    S={S:4d}"] = (S, lambda qkv=qkv, out=out, dout=dout, lse=lse: ops.attention_bwd_qkv_stream(qkv, out, dout, H, scale, lse))
        cases[f"composed (own ops)   S={S:4d}"] = (S, lambda qkv=qkv, dout=dout: Fn._attention_bwd(qkv, dout, H, scale))
    times = {k: [] for k in cases}
    for _ in range(7):                      # interleaved rounds
        for k, (S, fn) in cases.items():
            times[k].append(timed(fn, n=10))
    lines += [f"attention backward, B x H = {B} x {H}, head dim 64, random data, 7 interleaved rounds of 10 calls; TFLOP/s on 10 S^2 64 FLOP per head",
              f"{'case':32s} {'median us':>10s} {'min us':>10s} {'TF/s (median)':>14s} {'TF/s (min)':>11s}"]
    med = {}
    for k, (S, _) in cases.items():
        t = sorted(times[k])
        med[k], mn, fl = t[len(t) // 2], t[0], 10.0 * B * H * S * S * D
        lines.append(f"{k:32s} {med[k]:10.1f} {mn:10.1f} {fl / med[k] * 1e-6:14.1f} {fl / mn * 1e-6:11.1f}")
    for S in (577, 1025):
        lines.append(f"S={S}: composed / streaming (median) = {med[f'composed (own ops)   S={S:4d}'] / med[f'streaming kernels    S={S:4d}']:.2f}")
    del cases
    torch.cuda.empty_cache()
    # one trainable ViT-L block, forward + backward at 1025 tokens: peak allocation of the backward over what is allocated when it starts
    from dmvae_amd.models.vit import DinoV2ViT
    torch.manual_seed(0)
    blk = DinoV2ViT(embed_dim=1024, depth=1, num_heads=16, patch_size=8, img_size=256).cuda().blocks[0]
    Bv, S = 16, 1025
    t0 = torch.randn(Bv, S, 1024, device="cuda", generator=g)
    dy = torch.randn(Bv, S, 1024, device="cuda", generator=g)

    def block_backward_peak():
        t = t0.clone().requires_grad_(True)
        y = Fn.VitBlockFn.apply(t, blk.norm1.weight, blk.norm1.bias, blk.attn.qkv.weight, blk.attn.qkv.bias, blk.attn.proj.weight, blk.attn.proj.bias, blk.ls1.gamma,
                                blk.norm2.weight, blk.norm2.bias, blk.mlp.fc1.weight, blk.mlp.fc1.bias, blk.mlp.fc2.weight, blk.mlp.fc2.bias, blk.ls2.gamma,
                                blk.attn.num_heads, blk.norm1.eps)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y.backward(dy)
        torch.cuda.synchronize()
        blk.zero_grad(set_to_none=True)
        return (torch.cuda.max_memory_allocated() - before) / 2 ** 20

    block_backward_peak()                   # first call: workspaces and parameter gradients' buffers
    peak_stream = block_backward_peak()
    kernel_route = ops.attention_bwd_qkv
    ops.attention_bwd_qkv = lambda qkv, out, dout, heads, scale, lse=None: Fn._attention_bwd(qkv, dout, heads, scale)
    try:
        block_backward_peak()
        peak_comp = block_backward_peak()
    finally:
        ops.attention_bwd_qkv = kernel_route
    lines.append("")
    lines.append(f"one trainable ViT-L block (VitBlockFn) at {S} tokens, B = {Bv}: peak allocation of the backward above its starting point")
    lines.append(f"{'streaming attention backward':32s} {peak_stream:10.1f} MiB")
    lines.append(f"{'composed attention backward':32s} {peak_comp:10.1f} MiB   (difference {peak_comp - peak_stream:.1f} MiB)")
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


# ---- LightningDiT's head-major attention beyond 288 tokens ----------------------------------------------------------------------------------------------
def heads_stream_section(fwd, bwd, out_path):
    import torch.nn.functional as F
    B, H = 16, 16
    cases, lines = {}, []
    for D in (72, 64):
        DP, scale = (D + 31) // 32 * 32, D ** -0.5
        for N in (576, 1024):
            q, k = (F.pad(torch.randn(B * H, N, D, device="cuda", generator=g), (0, DP - D)).to(BF).contiguous() for _ in range(2))
            v = torch.randn(B * H, N, D, device="cuda", generator=g).to(BF)
            out, lse = ops.attention_heads_stream(q, k, v, B, scale, need_lse=True)
            tag = f"D={D} N={N:4d}"

            def comp_fwd(q=q, k=k, v=v, scale=scale):      # lightningdit_fast._attention / DitBlockFn.forward above the cap before the streaming kernels
                p = ops.softmax_rows(ops.gemm_nt(q, k, out_f32=True), scale)
                return p, ops.gemm_nt(p, ops.transpose_last2(v))
            p, oc = comp_fwd()
            a = out.view(B, N, H, D).permute(0, 2, 1, 3).reshape(B * H, N, D).float()
            lines.append(f"{tag}: streaming vs composed out rel-L2 {((a - oc.float()).norm() / oc.float().norm()).item():.2e}")
            if fwd:
                cases[f"fwd streaming + lse  {tag}"] = (4.0, D, N, lambda q=q, k=k, v=v, scale=scale: ops.attention_heads_stream(q, k, v, B, scale, need_lse=True))
                cases[f"fwd composed         {tag}"] = (4.0, D, N, comp_fwd)
            if bwd:
                dout = torch.randn(out.shape, device="cuda", generator=g).to(BF)
                do_h = dout.view(B, N, H, D).permute(0, 2, 1, 3).reshape(B * H, N, D).contiguous()
                do_p, v_p = (F.pad(do_h, (0, DP - D)), F.pad(v, (0, DP - D))) if DP > D else (do_h, v)

                def comp_bwd(q=q, k=k, p=p, do_h=do_h, do_p=do_p, v_p=v_p, scale=scale):      # DitBlockFn.backward's composed branch on the saved P
                    ds = ops.softmax_rows_bwd(ops.gemm_nt(do_p, v_p, out_f32=True), p, scale)
                    return ops.gemm_nt(ds, ops.transpose_last2(k)), ops.gemm_tn(ds, q), ops.gemm_tn(p, do_h)
                gs, gc = ops.attention_bwd_heads_stream(q, k, v, out, dout, B, scale, lse), comp_bwd()
                lines.append(f"{tag}: streaming vs composed " + "  ".join(f"{n_} rel-L2 {((x.float() - y.float()).norm() / y.float().norm()).item():.2e}"
                                                                            for n_, x, y in zip(("dq", "dk", "dv"), gs, gc)))
                del gs, gc
                cases[f"bwd streaming        {tag}"] = (10.0, D, N, lambda q=q, k=k, v=v, out=out, dout=dout, lse=lse, scale=scale:
                                                        ops.attention_bwd_heads_stream(q, k, v, out, dout, B, scale, lse))
                cases[f"bwd composed         {tag}"] = (10.0, D, N, comp_bwd)
            del p, oc, a
    rounds, calls = 7, 10
    times = {k_: [] for k_ in cases}
    for _ in range(rounds):                 # interleaved rounds
        for k_, (_, _, _, fn) in cases.items():
            times[k_].append(timed(fn, n=calls))
    lines += [f"LightningDiT attention on head-major operands, B x H = {B} x {H}, random data, {rounds} interleaved rounds of {calls} calls; TFLOP/s on 4 (forward) / 10 "
              f"(backward) N^2 D FLOP per head; composed = f32-score GEMM + row softmax + GEMM from this build's own ops, P saved for its backward",
              f"{'case':36s} {'median us':>10s} {'min us':>10s} {'max us':>10s} {'TF/s (median)':>14s}"]
    med = {}
    for k_, (fpp, D, N, _) in cases.items():
        t = sorted(times[k_])
        med[k_] = t[len(t) // 2]
        lines.append(f"{k_:36s} {med[k_]:10.1f} {t[0]:10.1f} {t[-1]:10.1f} {fpp * B * H * N * N * D / med[k_] * 1e-6:14.1f}")
    for k_ in cases:
        if "streaming" in k_:
            twin = k_.replace("streaming + lse", "composed       ").replace("streaming", "composed ")
            lines.append(f"{k_[:3]} {k_[-13:]}: composed / streaming (median) = {med[twin] / med[k_]:.2f}")
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


# ---- the decoder AttnBlock's attention: one head of 512 channels --------------------------------------------------------------------------------------------
def wide_section(out_path):
    from dmvae_amd import functional as Fn
    from dmvae_amd.models.flux_ae import AttnBlock
    B, C = 32, 512
    scale = C ** -0.5
    cases, lines = {}, []

    def comp_fwd(q, k, v):      # functional.AttnBlockFn's composed forward
        return ops.gemm_nt(ops.softmax_rows(ops.gemm_nt(q, k, out_f32=True), scale), ops.transpose_last2(v))
    for S in (2304, 4096, 1024):
        q, k, v = (torch.randn(B, S, C, device="cuda", generator=g).to(BF) for _ in range(3))
        a, c = ops.attention_wide_stream(q, k, v, scale).float(), comp_fwd(q, k, v).float()
        lines.append(f"S={S}: streaming vs composed out rel-L2 {((a - c).norm() / c.norm()).item():.2e}")
        del a, c
        cases[f"streaming + lse   S={S:4d}"] = (S, lambda q=q, k=k, v=v: ops.attention_wide_stream(q, k, v, scale, need_lse=True))
        cases[f"streaming, no lse S={S:4d}"] = (S, lambda q=q, k=k, v=v: ops.attention_wide_stream(q, k, v, scale))
        cases[f"composed          S={S:4d}"] = (S, lambda q=q, k=k, v=v: comp_fwd(q, k, v))
    rounds, calls = 7, 10
    times = {k_: [] for k_ in cases}
    for _ in range(rounds):                 # interleaved rounds
        for k_, (_, fn) in cases.items():
            times[k_].append(timed(fn, n=calls))
    lines += [f"decoder AttnBlock attention forward, one head of {C} channels, B = {B}, random data, {rounds} interleaved rounds of {calls} calls; TFLOP/s on 4 S^2 {C} FLOP "
              f"per sample; composed = gemm_nt (f32 scores) + softmax_rows + transpose_last2 + gemm_nt, this build's own ops",
              f"{'case':28s} {'median us':>10s} {'min us':>10s} {'max us':>10s} {'TF/s (median)':>14s}"]
    med = {}
    for k_, (S, _) in cases.items():
        t = sorted(times[k_])
        med[k_] = t[len(t) // 2]
        lines.append(f"{k_:28s} {med[k_]:10.1f} {t[0]:10.1f} {t[-1]:10.1f} {4.0 * B * S * S * C / med[k_] * 1e-6:14.1f}")
    for S in (2304, 4096, 1024):
        lines.append(f"S={S}: composed / streaming + lse (median) = {med[f'composed          S={S:4d}'] / med[f'streaming + lse   S={S:4d}']:.2f}")
    del cases, q, k, v
    torch.cuda.empty_cache()
    # one AttnBlock(512), forward + backward at 64 x 64 tokens: what the forward leaves allocated, and the peak of the whole, above the starting point
    torch.manual_seed(0)
    blk = AttnBlock(C).cuda()
    Bm, side = 8, 64
    x0 = torch.randn(Bm, side, side, C, device="cuda", generator=g).to(BF)
    dy = torch.randn(Bm, side, side, C, device="cuda", generator=g).to(BF)

    def block_alloc(route):
        Fn.ATTN_WIDE_STREAM = route
        try:
            x = x0.clone().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            y = blk.forward_nhwc(x)
            torch.cuda.synchronize()
            held, fwd_peak = torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before
            y.backward(dy)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - before
        finally:
            Fn.ATTN_WIDE_STREAM = None
        blk.zero_grad(set_to_none=True)
        return held / 2 ** 20, fwd_peak / 2 ** 20, peak / 2 ** 20
    lines.append("")
    lines.append(f"one AttnBlock({C}) at {side} x {side} = {side * side} tokens, B = {Bm}: MiB above the starting point (second call of each route; the first sizes the workspaces)")
    lines.append(f"{'route':28s} {'held after fwd':>15s} {'peak of fwd':>12s} {'peak fwd+bwd':>13s}")
    for name, route in (("streaming forward", True), ("composed forward", False)):
        block_alloc(route)
        held, fwd_peak, peak = block_alloc(route)
        lines.append(f"{name:28s} {held:15.1f} {fwd_peak:12.1f} {peak:13.1f}")
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


# ---- its backward ----------------------------------------------------------------------------------------------------------------------------------------------
def wide_bwd_section(out_path):
    from dmvae_amd import functional as Fn
    from dmvae_amd.models.flux_ae import AttnBlock
    B, C = 32, 512
    scale = C ** -0.5
    cases, lines = {}, []

    def comp_bwd(q, k, v, do):      # functional.AttnBlockFn's backward behind a streaming forward without the streaming backward: P recomputed, then the composed body
        p = Fn._attn_probs(q, k, scale, q.shape[1])
        ds = ops.softmax_rows_bwd(ops.gemm_nt(do, v, out_f32=True), p, scale)
        return ops.gemm_nt(ds, ops.transpose_last2(k)), ops.gemm_tn(ds, q), ops.gemm_tn(p, do)
    for S in (1024, 2304, 4096):
        q, k, v, do = (torch.randn(B, S, C, device="cuda", generator=g).to(BF) for _ in range(4))
        o, lse = ops.attention_wide_stream(q, k, v, scale, need_lse=True)
        gs, gc = ops.attention_wide_bwd_stream(q, k, v, o, do, lse, scale), comp_bwd(q, k, v, do)
        lines.append(f"S={S}: streaming vs composed " + "  ".join(f"{n_} rel-L2 {((x.float() - y.float()).norm() / y.float().norm()).item():.2e}"
                                                                 for n_, x, y in zip(("dq", "dk", "dv"), gs, gc)))
        del gs, gc
        cases[f"bwd streaming          S={S:4d}"] = (S, lambda q=q, k=k, v=v, o=o, do=do, lse=lse: ops.attention_wide_bwd_stream(q, k, v, o, do, lse, scale))
        cases[f"bwd composed recompute S={S:4d}"] = (S, lambda q=q, k=k, v=v, do=do: comp_bwd(q, k, v, do))
    rounds, calls = 7, 10
    times = {k_: [] for k_ in cases}
    for _ in range(rounds):                 # interleaved rounds
        for k_, (_, fn) in cases.items():
            times[k_].append(timed(fn, n=calls))
    lines += [f"decoder AttnBlock attention backward, one head of {C} channels, B = {B}, random data, {rounds} interleaved rounds of {calls} calls; TFLOP/s on 10 S^2 {C} "
              f"FLOP per sample; composed recompute = gemm_nt (f32 scores) + softmax_rows, gemm_nt (f32 dP) + softmax_rows_bwd, gemm_tn, transpose_last2 + gemm_nt, "
              f"gemm_tn, this build's own ops",
              f"{'case':32s} {'median us':>10s} {'min us':>10s} {'max us':>10s} {'TF/s (median)':>14s}"]
    med = {}
    for k_, (S, _) in cases.items():
        t = sorted(times[k_])
        med[k_] = t[len(t) // 2]
        lines.append(f"{k_:32s} {med[k_]:10.1f} {t[0]:10.1f} {t[-1]:10.1f} {10.0 * B * S * S * C / med[k_] * 1e-6:14.1f}")
    for S in (1024, 2304, 4096):
        lines.append(f"S={S}: composed recompute / streaming (median) = {med[f'bwd composed recompute S={S:4d}'] / med[f'bwd streaming          S={S:4d}']:.2f}")
    del cases, q, k, v, do, o, lse
    torch.cuda.empty_cache()
    # one AttnBlock(512), forward + backward at 64 x 64 tokens: what the forward leaves allocated, and the peaks, above the starting point
    torch.manual_seed(0)
    blk = AttnBlock(C).cuda()
    Bm, side = 8, 64
    x0 = torch.randn(Bm, side, side, C, device="cuda", generator=g).to(BF)
    dy = torch.randn(Bm, side, side, C, device="cuda", generator=g).to(BF)

    def block_alloc(fwd, bwd):
        Fn.ATTN_WIDE_STREAM, Fn.ATTN_WIDE_BWD_STREAM = fwd, bwd
        try:
            x = x0.clone().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            y = blk.forward_nhwc(x)
            torch.cuda.synchronize()
            held, fwd_peak = torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before
            y.backward(dy)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - before
        finally:
            Fn.ATTN_WIDE_STREAM, Fn.ATTN_WIDE_BWD_STREAM = None, None
        blk.zero_grad(set_to_none=True)
        return held / 2 ** 20, fwd_peak / 2 ** 20, peak / 2 ** 20
    lines.append("")
    lines.append(f"one AttnBlock({C}) at {side} x {side} = {side * side} tokens, B = {Bm}: MiB above the starting point (second call of each route; the first sizes the workspaces)")
    lines.append(f"{'route':44s} {'held after fwd':>15s} {'peak of fwd':>12s} {'peak fwd+bwd':>13s}")
    for name, fwd, bwd in (("streaming forward, streaming backward", None, None), ("streaming forward, composed recompute", None, False),
                           ("composed forward and backward", False, None)):
        block_alloc(fwd, bwd)
        held, fwd_peak, peak = block_alloc(fwd, bwd)
        lines.append(f"{name:44s} {held:15.1f} {fwd_peak:12.1f} {peak:13.1f}")
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if "--wide-bwd" in sys.argv:
    wide_bwd_section(OUT)
elif "--wide" in sys.argv:
    wide_section(OUT)
elif "--heads-stream" in sys.argv or "--heads-stream-bwd" in sys.argv:
    heads_stream_section("--heads-stream" in sys.argv, "--heads-stream-bwd" in sys.argv, OUT)
elif "--stream-bwd" in sys.argv:
    stream_bwd_section(OUT)
else:
    stream_section(OUT)
