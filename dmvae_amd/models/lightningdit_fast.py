"""Inference forward of LightningDiT on the HIP kernels (csrc/dit.hip) -- the route `LightningDiT.forward` takes when no gradient is needed
(the teacher's and the student's evaluations inside the DMD loss, train_dmd.py:211-217: four DiT-XL/1 forwards per VAE turn).

Same arithmetic as `forward_stock` under autocast(bf16), with bf16 rounding at the sites where the reference's autocast graph rounds (see
csrc/dit.hip); per block: 1 fused (gated residual +) RMSNorm+modulate, qkv GEMM, 1 fused QK-norm+RoPE+head split, attention in one fused kernel (csrc/attention.hip, head dims 64 and 72
alike: the staged head dim pads to 96; beyond 288 tokens QK-norm + RoPE as their own kernel and the streaming-softmax kernel of csrc/attention_stream.hip -- nothing N x N in
HBM at any token count; other head dims beyond 288 tokens: composed batched QK^T GEMM / f32 softmax / PV GEMM), proj GEMM, 1 gated residual, RMSNorm+modulate, w12 GEMM, SwiGLU gate, w3 GEMM,
gated residual -- every token-level Linear on this build's GEMM kernel (`functional.linear`: csrc/gemm_pp.hip).
The per-sample pieces (timestep / label embedding, adaLN Linear: one row per sample) stay stock PyTorch under autocast.

Block VARIANTS (the constructor's use_rmsnorm / wo_shift / use_swiglu / use_rope / use_qknorm away from their defaults; `variant_supported`) take the same two
routes with per-block choices: affine-free LayerNorm + modulate instead of RMSNorm, the 4-chunk adaLN row, the head split for {no norm, RMS} x {no RoPE, RoPE}
in front of `ops.attention_heads`, fc1 / tanh-GELU / fc2 instead of the SwiGLU pair (csrc/dit_variants.hip); training through the same `functional.DitBlockFn` as
the default block, whose absent parameters are None.  The default block issues the launches it always did."""
import os
from typing import Optional

import torch
import torch.nn.functional as F

from .. import ops
from .lightningdit import RMSNorm, SwiGLUFFN, _Mlp

_BF = torch.bfloat16


def _mlp(blk):
    """(is SwiGLU, first Linear, second Linear) of a block's MLP: w12 / w3 of `SwiGLUFFN`, fc1 / fc2 of the tanh-GELU `_Mlp`; None for any other module.  The inner
    width is the second Linear's in_features."""
    if isinstance(blk.mlp, SwiGLUFFN):
        return True, blk.mlp.w12, blk.mlp.w3
    if isinstance(blk.mlp, _Mlp):
        return False, blk.mlp.fc1, blk.mlp.fc2
    return None


def _shapes_supported(model) -> bool:
    """The shape limits of the DiT kernels, the same for the default block and the variants (`refused_reason` spells them out): width % 8 == 0 and <= 2048, even
    head dim <= 128, tokens a multiple of 32, MLP inner width % 8 == 0."""
    mlp = _mlp(model.blocks[0])
    c, hd = model.hidden_size, model.hidden_size // model.num_heads
    return bool(mlp is not None and c % 8 == 0 and c <= 2048 and hd % 2 == 0 and hd <= 128 and model.x_embedder.num_patches % 32 == 0
                and mlp[2].in_features % 8 == 0)


def structurally_supported(model) -> bool:
    """The configuration the DiT kernels cover (what `supported` checks besides the call's tensor and autocast state).  On this route every op is per sample
    -- per token row, per (sample, head) -- so a 2B-sample call equals two B-sample calls bit for bit (train.DMDTrainer's batched cond / uncond evaluation)."""
    blk = model.blocks[0]
    return bool(model.use_rope and model.use_rmsnorm and isinstance(blk.attn.q_norm, RMSNorm) and isinstance(blk.mlp, SwiGLUFFN) and not blk.wo_shift
                and _shapes_supported(model))


def variant_supported(model) -> bool:
    """A NON-default configuration of the constructor's five switches that the variant kernels (csrc/dit_variants.hip) cover, at the shape limits of
    `structurally_supported`: RMSNorm or affine-free LayerNorm, 6- or 4-chunk adaLN (`wo_shift`), SwiGLU or fc1 / tanh-GELU / fc2, with or without RoPE, RMS
    QK-norm or none.  Out: use_qknorm with use_rmsnorm=False (an affine nn.LayerNorm(head_dim) on q and k).  False for the default configuration: that is
    `structurally_supported`, which alone gates the fp32 parity mode, `DitStackFn`, the one-token route and the batched-adaLN path -- all of which assume the
    default block.  Per-sample like the default route: a 2B-sample call equals two B-sample calls bit for bit."""
    if structurally_supported(model):
        return False
    blk = model.blocks[0]
    norm_ok = isinstance(blk.norm1, RMSNorm) or (isinstance(blk.norm1, torch.nn.LayerNorm) and not blk.norm1.elementwise_affine)
    qk_ok = isinstance(blk.attn.q_norm, (RMSNorm, torch.nn.Identity))
    return bool(norm_ok and qk_ok and (model.feat_rope is not None) == bool(model.use_rope) and _shapes_supported(model))


def refused_reason(model) -> str:
    """What `LightningDiT.forward` names when it refuses a call: the configurations and shapes still outside the kernels."""
    blk = model.blocks[0]
    if isinstance(blk.attn.q_norm, torch.nn.LayerNorm):
        return ("use_qknorm=True with use_rmsnorm=False (an affine nn.LayerNorm(head_dim) on q and k): the one combination of the constructor's switches the DiT "
                "kernels do not cover")
    return ("call outside autocast(bfloat16), the fp32 parity mode with a non-default block, or a shape the DiT kernels do not cover (width % 8 == 0 and <= 2048, "
            "even head dim <= 128, tokens a multiple of 32, MLP inner width % 8 == 0)")


def supported(model, x: torch.Tensor) -> bool:
    if not (x.is_cuda and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == _BF):
        return False
    if x.shape[-1] * x.shape[-2] != model.x_embedder.num_patches * model.patch_size ** 2:
        return False
    return structurally_supported(model) or (variant_supported(model) and not _parity_on())


def _bf(p):
    """bf16 copy of a parameter, cached until it changes (functional._bf: in-place optimiser updates bump `_version`) -- the frozen teacher
    converts its 675 M parameters once, not on each of its two evaluations per step."""
    from ..functional import _bf as cached
    return cached(p)


BATCHED_ADALN = True      # forward_inference: every block's adaLN modulation Linear in one launch (False: one launch per block; tests compare)


def _parity_on() -> bool:
    from .. import parity
    return parity.on()


_FUSED_ATTN = True        # False: attention composed from batched GEMMs + softmax (tests compare)
_FUSED_QKNORM = True      # QK-norm + RoPE inside the attention kernel


def _attention(qkv, blk, rope, heads):
    b, n, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    qn, kn = blk.attn.q_norm, blk.attn.k_norm
    if isinstance(qn, torch.nn.Identity) or rope is None:
        # a variant (no QK-norm and / or no RoPE): its own head split (csrc/dit_variants.hip), then the attention kernels on the head-major operands
        nw = (None, None) if isinstance(qn, torch.nn.Identity) else (qn.weight, kn.weight)
        tabs = (None, None) if rope is None else (rope.freqs_cos, rope.freqs_sin)
        q, k, v = ops.head_split(qkv, heads, nw[0], nw[1], tabs[0], tabs[1], getattr(qn, "eps", 1e-6))
    elif _FUSED_ATTN and _FUSED_QKNORM and n <= ops.ATTENTION_RESIDENT_MAX and ops.attention_heads_supported(n, d):      # the QK-norm variant is resident-only
        return ops.attention_qknorm_rope(qkv, qn.weight, kn.weight, rope.freqs_cos, rope.freqs_sin, heads, qn.eps, d ** -0.5)
    else:
        q, k, v = ops.qknorm_rope(qkv, qn.weight, kn.weight, rope.freqs_cos, rope.freqs_sin, heads, qn.eps)
    if _FUSED_ATTN and ops.attention_heads_supported(n, d):
        return ops.attention_heads(q, k, v, b, d ** -0.5)
    from ..functional import _heads_attention
    return _heads_attention(q, k, v, b, d ** -0.5, fused=False)[0]               # composed: QK^T GEMM, f32 softmax, PV GEMM


def _t_embed(model, t: torch.Tensor, train: bool = False) -> torch.Tensor:
    """TimestepEmbedder.forward (lightningdit.py:96-139) under autocast(bf16) on this build's kernels: sinusoidal features (f32, cast like autocast casts a
    Linear's input) -> Linear -> SiLU (on the bf16-rounded pre-activation, in the GEMM's epilogue when no gradient is needed) -> Linear; bf16 [B, C]."""
    from ..functional import LinearFn, SiluFn, linear
    te = model.t_embedder
    emb = te.timestep_embedding(t, te.frequency_embedding_size)
    l0, l2 = te.mlp[0], te.mlp[2]
    if train:
        return LinearFn.apply(SiluFn.apply(LinearFn.apply(emb, l0.weight, l0.bias)), l2.weight, l2.bias)
    return linear(linear(emb.to(_BF), l0.weight, l0.bias, ops.ACT_SILU), l2.weight, l2.bias)


def _norm_modulate(norm, h, mod, shift_off, scale_off, pend=None):
    """norm + adaLN modulate of the residual stream h -> the next Linear's bf16 input, by the norm's kind: RMSNorm with weight (csrc/dit.hip) or affine-free
    LayerNorm (csrc/dit_variants.hip).  pend = (y, its adaLN row, its gate offset): the gated residual not yet added to h, folded into the same pass (h in place)."""
    if getattr(norm, "weight", None) is not None:
        if pend is None:
            return ops.rmsnorm_modulate(h, norm.weight, mod, shift_off, scale_off, norm.eps)
        return ops.gated_residual_rmsnorm_modulate_(h, pend[0], pend[1], pend[2], norm.weight, mod, shift_off, scale_off, norm.eps)
    if pend is None:
        return ops.layernorm_modulate(h, mod, shift_off, scale_off, norm.eps)
    return ops.gated_residual_layernorm_modulate_(h, pend[0], pend[1], pend[2], mod, shift_off, scale_off, norm.eps)


@torch.no_grad()
def forward_inference(model, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x [B,C,H,W], t [B], y [B] -> velocity [B,C_out,H,W] in bf16 (what the stock modules return under autocast)."""
    from ..functional import linear
    b, cin, hh, ww = x.shape
    ps, c, heads = model.patch_size, model.hidden_size, model.num_heads
    w = model.x_embedder.proj.weight
    patches = x.view(b, cin, hh // ps, ps, ww // ps, ps).permute(0, 2, 4, 1, 3, 5).reshape(b, -1, cin * ps * ps)
    h = linear(patches.to(_BF), _bf(w).view(w.shape[0], -1), _bf(model.x_embedder.proj.bias)).float() + model.pos_embed
    h = h.contiguous()
    n = h.shape[1]
    cvec = _t_embed(model, t) + model.y_embedder(y, False)                      # [B, C] f32: bf16 timestep embedding + the f32 label-embedding row
    sc = F.silu(cvec)
    # Every gated residual is folded into the RMSNorm that follows it (one pass over the residual stream instead of two), so a block's MLP residual is applied
    # by the NEXT block's norm1 -- or by the final layer's norm -- with that layer's modulation.
    scb = sc.to(_BF)
    fl = model.final_layer

    def adaln(lin):
        # [B, 6C]: shift_msa | scale_msa | gate_msa | shift_mlp | scale_mlp | gate_mlp.  One row per SAMPLE (16-64 rows against a 6912 x 1152 weight): a
        # GEMV-shaped, weight-bandwidth-bound problem -- `linear` sends it to the weight-streaming kernel (csrc/linear_rows.hip); more than 64 samples per call
        # go to the tile kernels
        return linear(scb, lin.weight, lin.bias)

    # the adaLN Linears of ALL blocks as one batched launch (csrc/linear_rows.hip, blockIdx.y = block): the same kernel and the same bits as one call per block
    lins = [blk.adaLN_modulation[1] for blk in model.blocks]
    mods = None
    if BATCHED_ADALN and lins and b <= 64 and ops.linear_rows_supported(b, lins[0].weight.shape[0], c) and not _parity_on():
        wb = [ww if ww.dtype == _BF else _bf(ww) for ww in (l.weight for l in lins)]
        bb = [bv if bv.dtype == _BF else _bf(bv) for bv in (l.bias for l in lins)]
        mods = ops.linear_rows_batched(scb, wb, bb)                               # [L, B, 6C]
    pend = None                                                                   # (y, mod, gate offset) of the previous block's MLP branch, not yet added to h
    from ..functional import dit_mod_offsets
    sh1, sc1, g1, sh2, sc2, g2 = dit_mod_offsets(c, bool(model.blocks) and model.blocks[0].wo_shift)      # the default block: 0, C, 2C, 3C, 4C, 5C
    for i, blk in enumerate(model.blocks):
        mod = mods[i] if mods is not None else adaln(blk.adaLN_modulation[1])
        a = _norm_modulate(blk.norm1, h, mod, sh1, sc1, pend)
        qkv = linear(a, blk.attn.qkv.weight, blk.attn.qkv.bias)
        o = linear(_attention(qkv, blk, model.feat_rope, heads), blk.attn.proj.weight, blk.attn.proj.bias)
        a = _norm_modulate(blk.norm2, h, mod, sh2, sc2, (o, mod, g1))
        swiglu, f1, f2 = _mlp(blk)
        if swiglu:
            g = linear(a, f1.weight, f1.bias, ops.ACT_SWIGLU)                      # silu(x1) * x2 in the GEMM's epilogue: x12 never reaches HBM
        else:                                                                      # fc1 -> tanh-GELU (its own pass, csrc/dit_variants.hip) -> fc2
            g = ops.gelu_tanh(linear(a, f1.weight, f1.bias).contiguous())
        pend = (linear(g, f2.weight, f2.bias), mod, g2)
    mod = adaln(fl.adaLN_modulation[1])                                           # [B, 2C]: shift | scale (the final layer always has its shift)
    a = _norm_modulate(fl.norm_final, h, mod, 0, c, pend)
    out = model.unpatchify(linear(a, fl.linear.weight, fl.linear.bias))
    if model.learn_sigma:
        out, _ = out.chunk(2, dim=1)
    return out


@torch.no_grad()
def forward_inference_cfg(model, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, cfg_scale: float, k: int, t_gate: Optional[torch.Tensor] = None,
                          interval_start: float = 0.0) -> torch.Tensor:
    """`LightningDiT.forward_with_cfg` (lightningdit.py:423-447) on the kernels: x [2n,C,H,W] whose first half is the latent of both halves, y [2n] = labels | null
    labels -> `forward_inference` at 2n, then ONE launch (`ops.cfg_combine`, csrc/sampler.hip) in place of the slices, sub, mul, add and two cats: the first k
    channels of both halves become uncond + cfg_scale * (cond - uncond), with the reference's bf16 rounding after each op (the same bits as the composition).
    `t_gate` (the model's t) switches the cfg_interval gate on: t_gate[0] < interval_start -> the conditional output, compared on the device -- no host read of
    t, so a guided sampler step can be captured in a graph."""
    half = x[: len(x) // 2]
    out = forward_inference(model, torch.cat([half, half], dim=0), t, y)
    return ops.cfg_combine(out.contiguous(), k, cfg_scale, t_gate, interval_start)


@torch.no_grad()
def forward_inference_autoguidance(model, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, cfg_scale: float, additional_model_forward,
                                   cfg_interval=(-1e4, -1e4)) -> torch.Tensor:
    """`LightningDiT.forward_with_autoguidance` (lightningdit.py:450-465) on the kernels: x [2n,C,H,W], t [2n], y [2n] whose first halves are used ->
    `forward_inference` and `additional_model_forward` on the n samples, then ONE launch (`ops.autoguidance_combine`, csrc/sampler.hip) in place of the two channel
    slices, sub, mul, add and the cat: [2n, in_channels, H, W] whose two halves hold ag + cfg_scale * (eps - ag) where cfg_interval[0] <= t[0] <= cfg_interval[1]
    and eps elsewhere, with the reference's rounding after each op.  The interval is compared on the device -- no host read of t, so the call can be captured in a
    graph.  The guide's output must be a CUDA tensor of this model's output type (bf16 under autocast): `ops.autoguidance_combine` refuses anything else."""
    half, th_, yh = x[: len(x) // 2], t[: len(t) // 2], y[: len(y) // 2]
    out = forward_inference(model, half, th_, yh)
    ag = additional_model_forward(half, th_, yh)
    return ops.autoguidance_combine(out.contiguous(), ag.contiguous(), model.in_channels, cfg_scale, th_, cfg_interval)


class GraphedInference:
    """`forward_inference` of a FROZEN model captured once in a hipGraph and replayed: `f(x, t, y)` copies the arguments into the graph's static inputs,
    replays ~330 kernel launches with one host call and returns the graph's static output buffer (overwritten by the next call -- consume it first).
    For loops that call the same model hundreds of times at one shape (the sampler: 250 steps per batch, where launching the kernels one by one
    leaves the GPU idle 10-15 % of the step).  Must be built and called under the autocast(bf16) context `forward_inference` needs.  The captured kernels
    read the cached bf16 copies of the weights: rebuild after the weights change."""

    def __init__(self, model, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, warmup: int = 2):
        if not supported(model, x):
            raise RuntimeError("GraphedInference needs the HIP inference route (CUDA tensors under torch.autocast('cuda', dtype=torch.bfloat16))")
        self.model = model
        self.x, self.t, self.y = x.detach().clone(), t.detach().clone(), y.detach().clone()
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side), torch.no_grad():                      # warm-up off the capture: lazy kernel attributes, GEMM heuristics, weight caches
            for _ in range(warmup):
                self._run()
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        # thread-local capture mode: in the default (global) mode every OTHER thread's event query is illegal while the capture lasts -- RCCL's watchdog thread
        # polls its work events all the time (sample_50k.py runs under torchrun) and aborts the process with "operation not permitted when stream is capturing"
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"), torch.no_grad():
            self.out = self._run()

    def _run(self) -> torch.Tensor:
        return forward_inference(self.model, self.x, self.t, self.y)

    def matches(self, x, t, y) -> bool:
        return x.shape == self.x.shape and x.dtype == self.x.dtype and t.shape == self.t.shape and y.shape == self.y.shape and x.device == self.x.device

    def __call__(self, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        assert GraphedInference.matches(self, x, t, y), "GraphedInference: shapes differ from the captured ones"
        self.x.copy_(x)
        self.t.copy_(t)
        self.y.copy_(y)
        self.graph.replay()
        return self.out


class GraphedInferenceCfg(GraphedInference):
    """The guided form: `forward_inference_cfg` captured at the [2n] shape -- the 2n-sample forward and the guidance kernel in one replay per model evaluation.
    Arguments after (x, t, y) are `LightningDiT.forward_with_cfg`'s; the guidance scale, the number of guided channels and the interval start are fixed at capture.
    `t` stays a static device input and the interval gate is evaluated by the kernel, so it follows the replayed t.  Called like `model.forward_with_cfg` (the
    sampler passes cfg_scale / standard_cfg / cfg_interval* as keywords): keywords that differ from the captured ones are an error, not ignored.  Same capture
    discipline, same lifetime of the returned buffer and the same rule about changed weights as `GraphedInference`."""

    def __init__(self, model, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, cfg_scale: float, cfg_interval=None, cfg_interval_start=None,
                 standard_cfg: bool = False, warmup: int = 2):
        if x.shape[0] % 2:
            raise ValueError("GraphedInferenceCfg: the batch is [cond | uncond], an even number of samples")
        self.cfg_scale, self.k = float(cfg_scale), int(model.in_channels if standard_cfg else 3)
        self.interval_start = float(cfg_interval_start) if cfg_interval is True else None
        super().__init__(model, x, t, y, warmup)

    def _run(self) -> torch.Tensor:
        gate = self.interval_start is not None
        return forward_inference_cfg(self.model, self.x, self.t, self.y, self.cfg_scale, self.k, self.t if gate else None, self.interval_start if gate else 0.0)

    def matches(self, x, t, y, cfg_scale, k, interval_start=None) -> bool:
        """Shapes as `GraphedInference.matches`, and the captured guidance: `cfg_scale`, `k` (guided channels), `interval_start` (None: gate off)."""
        return (super().matches(x, t, y) and float(cfg_scale) == self.cfg_scale and int(k) == self.k
                and (None if interval_start is None else float(interval_start)) == self.interval_start)

    def __call__(self, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, cfg_scale=None, cfg_interval=None, cfg_interval_start=None, standard_cfg=None) -> torch.Tensor:
        cfg_scale = self.cfg_scale if cfg_scale is None else cfg_scale
        k = self.k if standard_cfg is None else (self.model.in_channels if standard_cfg else 3)
        start = self.interval_start if cfg_interval is None else (cfg_interval_start if cfg_interval is True else None)
        assert self.matches(x, t, y, cfg_scale, k, start), "GraphedInferenceCfg: shapes or guidance settings differ from the captured ones"
        return GraphedInference.__call__(self, x, t, y)


class GraphedInferenceAutoguidance(GraphedInference):
    """Autoguidance as one replay per model evaluation: `forward_inference_autoguidance` captured at the [2n] shape -- this model's forward, the guide's
    (`additional_model_forward`, which must itself run on capturable kernels: a frozen LightningDiT's `forward` on the inference route) and the combine kernel, one
    after the other on the capturing stream (a single chain of nodes, no parallel branches).  The scale and the interval are fixed at capture; `t` stays a static
    device input and the kernel evaluates the interval, so it follows the replayed t.  Called like `model.forward_with_autoguidance` (the sampler passes cfg_scale /
    additional_model_forward / cfg_interval as keywords): keywords that differ from the captured ones are an error, not ignored.  Same capture discipline, same
    lifetime of the returned buffer and the same rule about changed weights (of either model) as `GraphedInference`."""

    def __init__(self, model, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, cfg_scale: float, additional_model_forward, cfg_interval=(-1e4, -1e4),
                 warmup: int = 2):
        if x.shape[0] % 2:
            raise ValueError("GraphedInferenceAutoguidance: the batch is [z | z], an even number of samples")
        self.cfg_scale, self.guide, self.interval = float(cfg_scale), additional_model_forward, (float(cfg_interval[0]), float(cfg_interval[1]))
        super().__init__(model, x, t, y, warmup)

    def _run(self) -> torch.Tensor:
        return forward_inference_autoguidance(self.model, self.x, self.t, self.y, self.cfg_scale, self.guide, self.interval)

    def matches(self, x, t, y, cfg_scale, additional_model_forward, cfg_interval) -> bool:
        """Shapes as `GraphedInference.matches`, and the captured guidance: scale, guide and interval."""
        return (super().matches(x, t, y) and float(cfg_scale) == self.cfg_scale and additional_model_forward == self.guide
                and (float(cfg_interval[0]), float(cfg_interval[1])) == self.interval)

    def __call__(self, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor, cfg_scale=None, additional_model_forward=None, cfg_interval=None) -> torch.Tensor:
        cfg_scale = self.cfg_scale if cfg_scale is None else cfg_scale
        guide = self.guide if additional_model_forward is None else additional_model_forward
        interval = self.interval if cfg_interval is None else cfg_interval
        assert self.matches(x, t, y, cfg_scale, guide, interval), "GraphedInferenceAutoguidance: shapes or guidance settings differ from the captured ones"
        return GraphedInference.__call__(self, x, t, y)


STACK_SEGMENTS = 1        # autograd nodes the block stack is cut into in a single process
STACK_SEGMENTS_DP = 4     # ... and with more than one rank (gradient buckets become ready per segment: the all-reduce overlaps the rest of the backward pass)
STACK_FN = True      # forward_train: all blocks as one functional.DitStackFn node (False: one DitBlockFn per block + LinearFn modulations; tests compare the two)


def tokens1_supported(model, x: torch.Tensor) -> bool:
    """The one-token configuration of the 2-D toy (toy_example_2d/dmd.py:436-454: LightningDiT-Mini/1 with input_size = 1): RoPE + RMSNorm + SwiGLU blocks, any
    SwiGLU width (682 there), width a multiple of 8, under autocast(bf16) on the GPU."""
    if not (x.is_cuda and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == _BF):
        return False
    blk = model.blocks[0]
    return bool(model.x_embedder.num_patches == 1 and x.shape[-1] * x.shape[-2] == model.patch_size ** 2 and model.use_rmsnorm and isinstance(blk.mlp, SwiGLUFFN)
                and isinstance(blk.norm1, RMSNorm) and not blk.wo_shift and model.hidden_size % 8 == 0 and model.hidden_size <= 2048)


def _swiglu_operands(blk):
    """w12 / b12 / w3 with the SwiGLU width H padded to a multiple of 32 -- rows [0, H) = x1's, [Hp, Hp + H) = x2's, the rest zero; w3's extra input columns zero --:
    LightningDiT-Mini's H = int(2/3 * 1024) = 682 is not a multiple of 8, the 16-byte granule of the bf16 kernels.  Padded columns give silu(0) * 0 = 0 and meet zero
    weights: the same function; torch.cat / pad are layout, their autograd slices the gradients back to the parameters' shapes."""
    w12, b12, w3 = blk.mlp.w12.weight, blk.mlp.w12.bias, blk.mlp.w3.weight
    h = w3.shape[1]
    hp = (h + 31) // 32 * 32
    if hp == h:
        return w12, b12, w3
    zw, zb = w12.new_zeros(hp - h, w12.shape[1]), b12.new_zeros(hp - h)
    return torch.cat([w12[:h], zw, w12[h:], zw]), torch.cat([b12[:h], zb, b12[h:], zb]), torch.nn.functional.pad(w3, (0, hp - h))


def forward_tokens1(model, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """LightningDiT.forward at ONE token per sample (config C1: every 2-D point is a [2, 1, 1] "image"), with or without gradients, on this build's kernels: with a
    single key the softmax is 1 and the attention output IS v -- q, k, their RMSNorm weights and RoPE do not reach the output and get exactly zero gradient, as in
    the reference --, so a block is five Linears (adaLN, qkv, proj, w12, w3) on the Linear GEMM kernels plus RMSNorm + modulate, the gated residuals and SwiGLU on
    csrc/dit.hip, composed from single autograd Functions (functional.LinearFn / RmsnormModulateFn / GatedResidualFn / SwigluFn).  The samples are the rows."""
    from ..functional import GatedResidualFn, LinearFn, RmsnormModulateFn, SwigluFn
    b, cin = x.shape[0], x.shape[1]
    ps, c = model.patch_size, model.hidden_size
    w = model.x_embedder.proj.weight
    train = torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters())
    h = (LinearFn.apply(x.reshape(b, 1, cin * ps * ps), w.view(w.shape[0], -1), model.x_embedder.proj.bias).float() + model.pos_embed).contiguous()
    cvec = _t_embed(model, t, train=train).float() + model.y_embedder(y, model.training)
    sc = F.silu(cvec)
    for blk in model.blocks:
        lin = blk.adaLN_modulation[1]
        mod = LinearFn.apply(sc, lin.weight, lin.bias)                              # [B, 6C] bf16
        a1 = RmsnormModulateFn.apply(h, blk.norm1.weight, mod, 0, c, blk.norm1.eps)
        v = LinearFn.apply(a1, blk.attn.qkv.weight, blk.attn.qkv.bias)[..., 2 * c:]   # attention over one key = its value
        h = GatedResidualFn.apply(h, LinearFn.apply(v.contiguous(), blk.attn.proj.weight, blk.attn.proj.bias), mod, 2 * c)
        a2 = RmsnormModulateFn.apply(h, blk.norm2.weight, mod, 3 * c, 4 * c, blk.norm2.eps)
        w12, b12, w3 = _swiglu_operands(blk)
        g = SwigluFn.apply(LinearFn.apply(a2, w12, b12))
        h = GatedResidualFn.apply(h, LinearFn.apply(g, w3, blk.mlp.w3.bias), mod, 5 * c)
    return _final_layer_train(model, h, sc)


def _final_layer_train(model, h: torch.Tensor, sc: torch.Tensor) -> torch.Tensor:
    """FinalLayer (lightningdit.py:260-273) with gradients on the residual stream h and sc = SiLU(conditioning): the adaLN Linear, the norm + modulate by the norm's
    kind (`RmsnormModulateFn`, or `LayernormModulateFn` for use_rmsnorm=False), the output Linear; then unpatchify and the `learn_sigma` split."""
    from ..functional import LayernormModulateFn, LinearFn, RmsnormModulateFn
    fl, c = model.final_layer, model.hidden_size
    mod = LinearFn.apply(sc, fl.adaLN_modulation[1].weight, fl.adaLN_modulation[1].bias)      # [B, 2C]: shift | scale (the final layer always has its shift)
    if getattr(fl.norm_final, "weight", None) is not None:
        a = RmsnormModulateFn.apply(h, fl.norm_final.weight, mod, 0, c, fl.norm_final.eps)
    else:
        a = LayernormModulateFn.apply(h, mod, 0, c, fl.norm_final.eps)
    out = model.unpatchify(LinearFn.apply(a, fl.linear.weight, fl.linear.bias))
    if model.learn_sigma:
        out, _ = out.chunk(2, dim=1)
    return out


def forward_train(model, x: torch.Tensor, t: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """`forward` with gradients (the student's flow-matching turn, train_dmd.py:565-575) under the caller's autocast(bf16): timestep / label embedders
    and the per-sample adaLN Linears through stock autograd, the patch embedding and the output Linear as `functional.LinearFn`, the blocks of the default
    configuration as `functional.DitStackFn` segments, else every block -- default or variant -- as one `functional.DitBlockFn` whose arguments are read off the
    block (an absent parameter is None), the final layer as `_final_layer_train`.  Label dropout as in the module (`y_embedder(y, model.training)`)."""
    from .. import functional as Fn
    from ..functional import DitBlockFn, DitStackFn, LinearFn
    Fn._OWNED_GRADS.clear()
    b, cin, hh, ww = x.shape
    ps, c, heads = model.patch_size, model.hidden_size, model.num_heads
    w = model.x_embedder.proj.weight
    patches = x.view(b, cin, hh // ps, ps, ww // ps, ps).permute(0, 2, 4, 1, 3, 5).reshape(b, -1, cin * ps * ps)
    h = (LinearFn.apply(patches, w.view(w.shape[0], -1), model.x_embedder.proj.bias).float() + model.pos_embed).contiguous()
    cvec = _t_embed(model, t, train=True).float() + model.y_embedder(y, model.training)      # the embedding lookup (and its index-add backward) is not a GEMM
    sc = F.silu(cvec)                                                             # adaLN_modulation[0] of every block: the same f32 values, computed once
    rope = model.feat_rope
    cos, sin = (None, None) if rope is None else (rope.freqs_cos, rope.freqs_sin)
    # `DitStackFn`, its grouped weight gradients and its stream-K scoping assume the default block
    stack = STACK_FN and structurally_supported(model) and Fn.dit_stack_supported(b, h.shape[1], c, heads)
    if stack:
        # One node per SEGMENT of blocks.  A single process takes all blocks as one segment; under data parallelism the gradients of a node reach autograd -- and
        # FlatGradSync's post-accumulate hooks, which start a bucket's all-reduce -- only when the node returns, so the stack is cut into STACK_SEGMENTS_DP nodes:
        # the collectives of the later blocks then run beside the backward pass of the earlier ones (2.7 GB of gradients for LightningDiT-XL/1, train_dmd.py:355)
        from .. import dist as _dist
        nseg = max(1, min(len(model.blocks), STACK_SEGMENTS_DP if _dist.get_world_size() > 1 else STACK_SEGMENTS))
        per = (len(model.blocks) + nseg - 1) // nseg
        for s0 in range(0, len(model.blocks), per):
            params = []
            for blk in model.blocks[s0:s0 + per]:
                params += [blk.norm1.weight, blk.attn.qkv.weight, blk.attn.qkv.bias, blk.attn.q_norm.weight, blk.attn.k_norm.weight, blk.attn.proj.weight,
                           blk.attn.proj.bias, blk.norm2.weight, blk.mlp.w12.weight, blk.mlp.w12.bias, blk.mlp.w3.weight, blk.mlp.w3.bias,
                           blk.adaLN_modulation[1].weight, blk.adaLN_modulation[1].bias]
            h = DitStackFn.apply(h, sc, cos, sin, heads, model.blocks[0].norm1.eps, *params)
    wt = lambda m: getattr(m, "weight", None)                                     # None: affine-free LayerNorm, no QK-norm (nn.Identity)
    for blk in (() if stack else model.blocks):
        lin = blk.adaLN_modulation[1]
        mod = LinearFn.apply(sc, lin.weight, lin.bias)                            # [B, 6C] or [B, 4C] bf16; one row per sample: csrc/linear_rows.hip forward and input gradient
        swiglu, f1, f2 = _mlp(blk)
        h = DitBlockFn.apply(h, mod, wt(blk.norm1), blk.attn.qkv.weight, blk.attn.qkv.bias, wt(blk.attn.q_norm), wt(blk.attn.k_norm), blk.attn.proj.weight,
                             blk.attn.proj.bias, wt(blk.norm2), f1.weight, f1.bias, f2.weight, f2.bias, cos, sin, heads, blk.norm1.eps, bool(blk.wo_shift), swiglu)
    return _final_layer_train(model, h, sc)
