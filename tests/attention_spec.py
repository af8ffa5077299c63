"""Not a test: the fp64 restatement of the resident attention kernels (csrc/attention.hip, csrc/attention_bwd.hip; S <= 288), the element-wise bars their outputs
are held to, the input classes, and f32 / bf16 emulations of the kernels in kernel order (tests/test_attention_spec_cpu.py, tests/test_gpu_attention_resident.py).
Nothing here needs a GPU or imports dmvae_amd; every function runs on the device of its operands.

Working layout: q, k, v, dO, o as [G, S, D] with G = batch * heads items (item g = b * H + h) and D the REAL head dim; `to_packed` / `to_heads` / `from_*` move
between it and the kernels' layouts (packed [B, S, 3, H, 64]; head-major q / k rows of D channels or of D rounded up to 32, zero-padded).

Definitions, float64 on the bf16 operands as given (x = scale q k^T):
  o = softmax(x) v      lse = logsumexp(x)      dv = P^T dO      dP = dO V^T      delta = rowsum(P o dP)      dS = P o (dP - delta)      dq = scale dS k      dk = scale dS^T q
The NR entry (attention_qknorm_rope) is dit_kernels_spec.qknorm_rope(rnd=True), its q / k rounded to bf16 as the kernel stages them, then the same definition.

Bars: |got - ref| <= bound per element, bound = 1.01 * 2^-8 * (|ref| + E) + E for a bf16 output (vit_kernels_spec.bf16_bound), E for the f32 lse.  E is a sum of
named terms, each a rounding site read from the kernel times the magnitude sum that site multiplies; u = 2^-8 (bf16), an f32 sum of n terms costs n * 2^-24 of
the sum of their magnitudes.  Nothing is fitted to what a kernel returns.  The sites:

  scores      s = q . k on the matrix cores, f32 sums of DP = 64 / 96 exact products:                    E_x = DP 2^-24 scale sum_d |q_d k_d|
  power       forward: 2^(fma(s, ec, -m ec)), ec = fl(scale fl(log2 e)) (2 roundings on |x|), the fma (1 on |x - xmax|); backward: 2^(fl(log2 e) (s scale - L)) -- the
              product (1 on |x|), the difference and the product with the rounded constant (3 on |x - L|).  One figure for both, per key:
                  eps_j = 2^-24 (3 |x_j| + 3 |x_j - xmax| + 2) + E_x_j          (+ 2: v_exp_f32 is good to 1 ulp = 2 * 2^-24, CDNA3 ISA guide, V_EXP_F32)
              what is common to a row's keys (the error of m, of m ec) cancels in P; it does not cancel in lse, below.
  row sum     the UNROUNDED e, 16 adds per key block in a lane and the half-wave swap:                   sum_depth = 16 nkb + 1
  lse         fl(fl(m scale) + logf(sum)): m scale (1) and m ec against it (3) on |xmax|; the sum's relative error; logf to 3 ulp (OpenCL C 7.4, the bound the
              compiler's expansion keeps) on log(sum) = lse - xmax; the add (1) on |lse|:
                  E_lse = 2^-24 (4 |xmax| + sum_depth + 6 (lse - xmax) + |lse|) + sum_j p_j eps_j
  out         e -> bf16 before P V while the sum keeps the unrounded e; P V an f32 sum of 32 nkb products; 1 / sum, the product, (3):
                  E_o = sum_j p_j (u + eps_j) |v_jd| + (sum_j p_j |v_jd|) (sum_j p_j eps_j + (32 nkb + sum_depth + 3) 2^-24)
  P backward  exp(scale s - L) with L the forward's f32 lse, itself within E_lse:  eps_b = eps_j + 3 * 2^-24 (lse - xmax) + E_lse
  dv          P -> bf16 before P^T dO, an f32 sum over 32 nblk queries:                                   E_dv = sum_q p_qj (u + eps_b + 32 nblk 2^-24) |dO_qd|
  delta       dO . O with O AS STORED in bf16 -- the forward's output, which lies within its own bar B_o of o:
                  E_delta = sum_d |dO_qd| B_o_qd + (D + 1) 2^-24 sum_d |dO_qd o_qd|
  dP          f32 sum of DP products:                                                                      E_dP = DP 2^-24 sum_d |dO_qd v_jd|
  dS          fl(fl(P (dP - delta)) scale) -> bf16 before both dS K and dS^T Q (T = scale p |dP - delta|):
                  W_qj = T_qj (u + eps_b + 4 * 2^-24) + scale p_qj (E_dP + E_delta)
  dq, dk      E_dq = sum_j (W_qj + 32 nblk 2^-24 T_qj) |k_jd|;  E_dk the same over q with |q_qd|
The kernel without lse takes its own max and sum; its L = fl(m + logf(sum)) and its e / sum go through the same sites (the fused exponent's terms are a superset),
so it is held to the same bars.

The NR entry's extra term.  The kernel's sum of squares of a row is an f32 sum in butterfly order, so bf16(x r) and the staged bf16 value can land on the other
neighbour where the fp64 value sits within TIE = 2^-19 (dit_kernels_spec.TIE: under 16 roundings on the way) of a rounding boundary.  `nr_operands` returns the
staged q / k the definition takes and dq_, dk_ >= the distance to any value the kernel may stage (zero away from ties); `bars_forward(..., dqk=)` carries them to
the scores, Dx_qj = scale sum_d (dq_ |k| + |q| dk_ + dq_ dk_), and to the output: sum_j p_j Dx_qj |v_jd| + (sum_j p_j Dx_qj) sum_j p_j |v_jd|, times
exp(2 max Dx) for the higher orders.

Worst |error| / bound of the emulations over every shared case (tests/test_attention_spec_cpu.py prints them; the only arbiter the bars have): out 0.744, lse 0.065,
dq 0.334, dk 0.388, dv 0.876; NR out 0.574.  No bar needed widening; the negative controls and what each reaches are listed in that module's docstring.

The streaming kernels (csrc/attention_stream.hip, csrc/attention_bwd_stream.hip; any S) compute the same operation and take the same `reference`; the second half of
this file holds THEIR bars (bars_forward_stream, bars_backward_stream: the derivation stands in the comment above them -- the per-tile alpha and emc sites, the row-sum
and P V depths per tile, delta as an output, both kinds of backward operands), three more input classes (ascending, descending, spike_last), the token counts at which
one of their mechanisms changes (STREAM_TOKENS) and their emulations with the tile walk (emulate_forward_stream, emulate_backward_stream).  The resident bars, classes
and emulations above are untouched by it.  Worst |error| / bound of the streaming emulations (tests/test_attention_stream_spec_cpu.py): out 0.726, lse 0.063; backward
on the forward's own out / lse dq 0.243, dk 0.295, dv 0.834, delta 0.170; on bf16(o) / f32(lse) of the definition dq 0.433, dk 0.529, dv 0.886, delta 0.353.

The d = 512 streaming kernels (csrc/attention_wide.hip, csrc/attention_wide_bwd.hip; one head, any S) take the same `reference` again; the third section of this file
holds THEIR bars (bars_forward_wide, bars_backward_wide: the derivation stands in the comment above them -- 512-channel scores, quarter sums in the backward, 32-key
tiles, delta = sum_k P dP from the kernel's own p with no term of the stored O, scale dS as hi + lo), the token counts (WIDE_TOKENS), make_case's `tile` parameter
(32 here; 64 by default, so every earlier case keeps its bits) and the emulations with the 32-key tile walk (emulate_forward_wide, emulate_backward_wide).
Worst |error| / bound, emulations (tests/test_attention_wide_spec_cpu.py) | MI355X (tests/test_gpu_attention_wide_spec.py):
  out 0.612 | 0.491, lse 0.022 | 0.042; backward on the forward's own lse dq 0.826 | 0.846, dk 0.687 | 0.698, dv 0.660 | 0.646, delta 0.012 | 0.013;
  on f32(lse) of the definition dq 0.829 | 0.848, dk 0.869 | 0.869, dv 0.750 | 0.751, delta 0.030 | 0.021.  No bar needed widening.
Negative controls, one changed line of an emulation each, and the bar each leaves (|error| / bound):
  leak out 108 (negative S 33), lse 26 (zeroq S 1025); mask_ignores_half out 117 (negative S 17); alpha_o_only lse 9.6e3 (ascending S 97); alpha_l_only out 1.2e6
  (last S 97); half_max lse 3.1e4 (spike S 33); lse_half lse 1.8e5 (zeroq S 33); l_rounded lse 2.5 (negative S 33); stale_tile out 1.7e5 (randn4 S 97);
  delta_from_O delta 33 / 40, dq 19 / 21 (last S 1025; own / made lse); ds_single_bf16 dq 3.9 (zeroq S 33), 3.5 (randn S 97), dk 2.7 (last S 33);
  quarter_dropped dq 716, dk 671, dv 861, delta 921 (randn S 97); p_from_max dq 2.8e7 (zeroq S 1025); dk_noscale dk 3.8e3 (last S 33); skip_one_q delta 1.6e3
  (last S 33), dq 1.0e3 (zeroq S 33); skip_one_k dv 105, dk 128 (randn S 33).  None is left "not told".
  Inert (neither): pad_key_unselected and pad_query_finite_L.  Padded K, V, Q and dO rows are staged as zeros, so the p a padded key or query keeps (finite: L > -88
  in every class) meets dP = 0 in delta's fmaf and zero rows in dQ, dK and dV: it adds +-0.  The emulations' outputs are bit-identical with and without (asserted).
  What the wide bars do NOT see: one leaked key on randn at 1025 tokens (lse 0.17) -- at 512 channels the scores' worst-case f32 term is as wide as that leak; zeroq,
  negative and offset at 1025 tokens are what see it."""
import math

import torch

import dit_kernels_spec as DS
from vit_kernels_spec import BF, D64, F32, FIG, TINY, U8, U24, bf16_bound, hold, note  # noqa: F401

RESIDENT_MAX = 288
LOG2E_F32 = 1.4426950408889634          # rounded to f32 where the kernels use it
TOKENS = [1, 31, 32, 33, 64, 65, 129, 200, 256, 257, 272, 288]
ALL_CLASS_TOKENS = (33, 257, 288)
CLASSES = ["randn", "negative", "randn4", "last", "zeroq", "offset", "spike"]
HEAD_FORMS = [(40, 40), (40, 64), (64, 64), (72, 72), (72, 96), (96, 96)]      # (head dim, channels a q / k row holds)
# the streaming kernels (any S; the second half of this file): 64-key tiles, the token counts at which one of their mechanisms changes, three more classes
STREAM_TILE = 64
STREAM_TOKENS = [1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 255, 256, 257, 289, 320, 321, 513, 577]
STREAM_ALL_CLASS_TOKENS = (257, 289, 320)          # one live key in the last tile, a ragged last tile, whole tiles
STREAM_CLASSES = CLASSES + ["ascending", "descending", "spike_last"]
STREAM_EVERYWHERE = ["randn", "negative", "ascending", "last"]
STREAM_HEAD_FORMS = [(64, 64), (72, 72), (72, 96)]
# the d = 512 streaming kernels (single head, any S; the third section of this file): 32-key tiles, 64-query forward blocks, 32-row backward blocks
WIDE_TILE = 32
WIDE_D = 512
WIDE_TOKENS = [1, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 128, 129, 1025, 1296]
WIDE_ALL_CLASS_TOKENS = (33, 97, 1025)          # one live key / row in the last tile: inside the first forward block, with an idle wave pair, and far out


def classes_at(s):
    return CLASSES if s in ALL_CLASS_TOKENS else CLASSES[:2]


def staged(d):
    return (d + 31) // 32 * 32


def nblocks(s):
    return (s + 31) // 32


def ntiles(s, tile=STREAM_TILE):
    return (s + tile - 1) // tile


def stream_classes_at(s):
    return STREAM_CLASSES if s in STREAM_ALL_CLASS_TOKENS else STREAM_EVERYWHERE


def wide_classes_at(s):
    return STREAM_CLASSES if s in WIDE_ALL_CLASS_TOKENS else STREAM_EVERYWHERE


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def spike_key(s):
    """the last key held by the upper half-wave of the forward's score registers (key % 8 >= 4); the last key where there is none"""
    c = [j for j in range(s) if j % 8 >= 4]
    return c[-1] if c else s - 1


def make_case(kind, b, h, s, d, seed=0, tile=STREAM_TILE):
    """-> dict of q, k, v, do [G, S, D] bf16 on the CPU, scale = d ** -0.5.  Classes (u: one unit direction per item, r = sqrt(d) / 8 so that scores are those of d = 64):
    randn (x 1.5), randn4 (x 4: peaked rows);
    negative  q = -g u, k = c u, g in [14, 16], c in sqrt(d) [0.62, 1] (d = 64: [4.96, 8]): every scaled score in [-16, -8.6] -- a key left at score 0 takes the weight
              (with a unit u, c below 4.6 would put scores above -8 and the class's own assertion would fail);
    last      q = g u, k = 0.2 linspace(0, 8) r u but the last key 8 r u: the last key takes >= 0.99 of every row (the only live key of its block at S = 32 k + 1);
    zeroq     zero queries: uniform rows, o = mean V, lse = log S;
    offset    k = a u + 0.1 randn, q = +- a u + 0.5 randn with scale a^2 = 80: |lse| ~ 80, where an f32 ulp is 8e-6;
    spike     keys 0.05 r u but key spike_key(S) = 56 r u, q = g u: that key scores ~105 against < 1, so a row maximum that misses it overflows the power.
    The streaming kernels' three (nt = ceil(S / tile) tiles, tile(j) = j // tile; tile = 64, or 32 for the d = 512 kernels):
    ascending   q = g u, k_j = 8 (tile(j) + 1) / nt jit_j r u, jit in [0.9, 1] and 1 on the last live key of each tile: every tile raises the running maximum by
                g / nt >= 0.8, so every tile's factor is < 1 and what tile 0 accumulated is rescaled nt - 1 times;
    descending  the same with (nt - tile(j)) / nt: the first tile holds the maximum and every later factor is exactly 1;
    spike_last  spike with the large key on S - 1, the last live key of the last tile.
    With 32-key tiles the same 16 units of score are climbed in up to 41 steps (S = 1296): a step is g / nt >= 0.34 there, see check_class."""
    g = _gen(STREAM_CLASSES.index(kind), b, h, s, d, seed)
    G = b * h
    rn = lambda *sh: torch.randn(*sh, generator=g)
    u = rn(G, 1, d)
    u = u / u.norm(dim=-1, keepdim=True)
    r = math.sqrt(d) / 8
    gq = 14 + 2 * torch.rand(G, s, 1, generator=g)
    v = rn(G, s, d) * 1.5
    if kind == "randn":
        q, k = rn(G, s, d) * 1.5, rn(G, s, d) * 1.5
    elif kind == "randn4":
        q, k, v = rn(G, s, d) * 4, rn(G, s, d) * 4, rn(G, s, d) * 4
    elif kind == "negative":
        q, k = -gq * u, math.sqrt(d) * (0.62 + 0.38 * torch.rand(G, s, 1, generator=g)) * u
    elif kind == "last":
        coef = torch.linspace(0, 8, s).view(1, s, 1) * 0.2
        coef[:, -1] = 8.0
        q, k = gq * u, coef * r * u
    elif kind == "zeroq":
        q, k = torch.zeros(G, s, d), rn(G, s, d) * 1.5
    elif kind == "offset":
        a = math.sqrt(80 * math.sqrt(d))
        sign = (torch.rand(G, s, 1, generator=g) < 0.5).double() * 2 - 1
        q, k = (sign * a * u + 0.5 * rn(G, s, d)).float(), a * u + 0.1 * rn(G, s, d)
    elif kind == "spike":
        coef = torch.full((1, s, 1), 0.05)
        coef[:, spike_key(s)] = 56.0
        q, k = gq * u, coef * r * u
    elif kind == "spike_last":
        coef = torch.full((1, s, 1), 0.05)
        coef[:, s - 1] = 56.0
        q, k = gq * u, coef * r * u
    elif kind in ("ascending", "descending"):
        nt, tj = ntiles(s, tile), torch.arange(s) // tile
        level = ((tj + 1) if kind == "ascending" else (nt - tj)).double() / nt
        jit = 0.9 + 0.1 * torch.rand(G, s, 1, generator=g)
        jit[:, torch.clamp((tj + 1) * tile, max=s) - 1] = 1.0          # the last live key of each tile
        q, k = gq * u, (8 * level.view(1, s, 1) * jit * r * u).float()
    else:
        raise ValueError(kind)
    return dict(kind=kind, b=b, h=h, s=s, d=d, tile=tile, scale=d ** -0.5, q=q.to(BF), k=k.to(BF), v=v.to(BF), do=rn(G, s, d).to(BF))


def check_class(c, ref):
    """the assertion ON THE REFERENCE ALONE that a class does what it is for"""
    kind, s, tile = c["kind"], c["s"], c.get("tile", STREAM_TILE)
    x = ref["x"]
    if kind == "negative":
        assert float(x.max()) <= -8.0, float(x.max())
    elif kind == "last":
        assert float(ref["p"][..., -1].min()) >= 0.99, float(ref["p"][..., -1].min())
    elif kind == "zeroq":
        assert float((ref["o"] - c["v"].double().mean(1, keepdim=True)).abs().max()) < 1e-12 and float((ref["lse"] - math.log(s)).abs().max()) < 1e-12
    elif kind == "offset":
        assert float(ref["lse"].abs().min()) >= 60.0, float(ref["lse"].abs().min())
    elif kind in ("ascending", "descending") and ntiles(s, tile) > 1:
        tm = tile_max(x, tile)
        if kind == "ascending":      # every tile after the first raises the maximum by at least 0.5
            gap = (tm[..., 1:] - torch.cummax(tm, -1).values[..., :-1]).min()
        else:                        # the first tile holds the maximum, at least 0.5 above every later tile's
            gap = (tm[..., :1] - tm[..., 1:]).min()
        # 64-key tiles: 0.5 as ever.  32-key tiles: the step is g / nt with g >= 14 and nt up to 41; q and k are rounded to bf16, 2 * 2^-9 of a score of at
        # most 16.1 = 0.063 on either side of a step, so 14 / nt - 0.13 is kept and 0.6 * 14 / nt asked (0.20 at 1296 tokens: a factor of exp(-0.2) = 0.82)
        need = 0.5 if tile == STREAM_TILE else min(0.5, 0.6 * 14 / ntiles(s, tile))
        assert float(gap) >= need, (float(gap), need)
    elif kind in ("spike", "spike_last") and s > 1:
        j = spike_key(s) if kind == "spike" else s - 1
        rest = torch.cat([x[..., :j], x[..., j + 1:]], -1)
        assert float((x[..., j] - rest.max(-1).values).min()) >= 96.0      # > log(FLT_MAX) = 88.7
        assert float(ref["p"][..., j].min()) >= 1 - 1e-30


def tile_max(x, tile=STREAM_TILE):
    """[.., S] scaled scores -> [.., nt]: the maximum of every `tile`-key tile"""
    s, nt = x.shape[-1], ntiles(x.shape[-1], tile)
    pad = torch.full(x.shape[:-1] + (nt * tile,), float("-inf"), dtype=x.dtype, device=x.device)
    pad[..., :s] = x
    return pad.view(*x.shape[:-1], nt, tile).max(-1).values


def to_dev(c, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------
def to_packed(q, k, v, b, h):
    """[G, S, D] x 3 -> [B, S, 3 H D] (the qkv Linear's output)"""
    G, s, d = q.shape
    return torch.stack([t.view(b, h, s, d) for t in (q, k, v)], 0).permute(1, 3, 0, 2, 4).reshape(b, s, 3 * h * d).contiguous()


def from_packed(t, b, h):
    """[B, S, 3 H D] -> three [G, S, D]"""
    s, d = t.shape[1], t.shape[2] // (3 * h)
    x = t.view(b, s, 3, h, d).permute(2, 0, 3, 1, 4).reshape(3, b * h, s, d)
    return x[0], x[1], x[2]


def to_rows(t, b, h):
    """[G, S, D] -> [B, S, H D] (out / dout)"""
    G, s, d = t.shape
    return t.view(b, h, s, d).permute(0, 2, 1, 3).reshape(b, s, h * d).contiguous()


def from_rows(t, b, h):
    s, d = t.shape[1], t.shape[2] // h
    return t.view(b, s, h, d).permute(0, 2, 1, 3).reshape(b * h, s, d)


def pad_rows(t, width):
    """[G, S, D] -> [G, S, width], zero-padded"""
    G, s, d = t.shape
    if width == d:
        return t.contiguous()
    o = torch.zeros(G, s, width, dtype=t.dtype, device=t.device)
    o[..., :d] = t
    return o


# ---- definitions -----------------------------------------------------------------------------------------------------------------------------
def reference(q, k, v, do, scale):
    """fp64 on the operands as given -> dict x, lse, p, o, dv, dP, delta, dq, dk"""
    q, k, v, do = q.double(), k.double(), v.double(), do.double()
    x = scale * q @ k.transpose(-1, -2)
    lse = torch.logsumexp(x, -1)
    p = torch.exp(x - lse.unsqueeze(-1))
    o = p @ v
    dP = do @ v.transpose(-1, -2)
    delta = (p * dP).sum(-1, keepdim=True)
    dS = p * (dP - delta)
    return dict(x=x, lse=lse, p=p, o=o, dv=p.transpose(-1, -2) @ do, dP=dP, delta=delta, dq=scale * dS @ k, dk=scale * dS.transpose(-1, -2) @ q)


def bars_forward(q, k, v, scale, ref, dqk=None):
    """-> dict o (bound on the bf16 out), lse (bound on the f32 lse), and the pieces the backward bars reuse"""
    s, d = q.shape[-2:]
    dp, nkb = staged(d), nblocks(s)
    qa, ka, va = q.double().abs(), k.double().abs(), v.double().abs()
    x, p, lse = ref["x"], ref["p"], ref["lse"]
    xmax = x.max(-1, keepdim=True).values
    e_x = dp * U24 * scale * qa @ ka.transpose(-1, -2)
    eps = U24 * (3 * x.abs() + 3 * (x - xmax).abs() + 2) + e_x
    sum_depth = 16 * nkb + 1
    peps = (p * eps).sum(-1, keepdim=True)
    lsum = (lse.unsqueeze(-1) - xmax)                                    # log(sum) >= 0
    e_lse = (U24 * (4 * xmax.abs() + sum_depth + 6 * lsum + lse.unsqueeze(-1).abs()) + peps).squeeze(-1)
    a = p @ va
    e_o = (p * (U8 + eps)) @ va + a * (peps + (32 * nkb + sum_depth + 3) * U24) + TINY
    if dqk is not None:
        dq_, dk_ = dqk
        dx = scale * (dq_ @ ka.transpose(-1, -2) + qa @ dk_.transpose(-1, -2) + dq_ @ dk_.transpose(-1, -2))
        e_o = e_o + ((p * dx) @ va + (p * dx).sum(-1, keepdim=True) * a) * torch.exp(2 * dx.max())
    return dict(o=bf16_bound(ref["o"], e_o), lse=e_lse + TINY, eps=eps, xmax=xmax, e_lse=e_lse)


def bars_backward(q, k, v, do, scale, ref, fwd):
    """-> dict dq, dk, dv (bounds on the bf16 gradients); fwd = bars_forward(...) of the same operands: O as stored lies within fwd['o'] of o, L within fwd['lse']"""
    s, d = q.shape[-2:]
    dp, nblk = staged(d), nblocks(s)
    qa, ka, va, da = q.double().abs(), k.double().abs(), v.double().abs(), do.double().abs()
    x, p, lse = ref["x"], ref["p"], ref["lse"].unsqueeze(-1)
    eps_b = fwd["eps"] + 3 * U24 * (lse - fwd["xmax"]) + fwd["e_lse"].unsqueeze(-1)
    depth = 32 * nblk * U24
    e_dv = (p * (U8 + eps_b + depth)).transpose(-1, -2) @ da + TINY
    e_delta = (da * fwd["o"]).sum(-1, keepdim=True) + (d + 1) * U24 * (da * ref["o"].abs()).sum(-1, keepdim=True)
    e_dp = dp * U24 * da @ va.transpose(-1, -2)
    t = scale * p * (ref["dP"] - ref["delta"]).abs()
    w = t * (U8 + eps_b + 4 * U24) + scale * p * (e_dp + e_delta) + depth * t
    return dict(dq=bf16_bound(ref["dq"], w @ ka + TINY), dk=bf16_bound(ref["dk"], w.transpose(-1, -2) @ qa + TINY), dv=bf16_bound(ref["dv"], e_dv))


def ratio(got, ref, bound):
    """worst |got - ref| / bound; inf where anything is not finite"""
    err = (got.double() - ref).abs()
    r = (err / bound.clamp_min(1e-300)).nan_to_num(float("inf"), posinf=float("inf"))
    return float(r.max()) if r.numel() else 0.0


# ---- the NR entry's operands -----------------------------------------------------------------------------------------------------------------
NR_DEPTH = 8      # the staged value: bf16(x r) * w (1), two products and the sum per rotated pair (3), r = rsqrt(ss / D + eps) carried through bf16(x r) is the tie term; taken as 8


def nr_operands(qkv, qw, kw, cos, sin, heads, eps):
    """qkv [B, N, 3 H D] bf16, f32 weights and tables -> (q, k, v [G, N, D] bf16 as the definition takes them: the fp64 qknorm_rope values rounded to bf16,
    dq_, dk_ [G, N, D] fp64: how far a correctly working kernel's staged value may lie from them).  A value moves only where bf16(x r) or the staged rounding
    sits within TIE (plus the f32 work on the rotated pair) of a boundary: the interval of values the kernel may round, pushed through bf16 at both ends."""
    qv, kv, tq, tk, v = DS.qknorm_rope(qkv, qw, kw, cos, sin, heads, eps, rnd=True)
    t, d = DS._heads(qkv, heads)
    b, n = qkv.shape[:2]
    cosd, sind = cos.double(), sin.double()

    def slack(u, w, val, terms):
        nh = u * torch.rsqrt(u.pow(2).mean(-1, keepdim=True) + eps)
        da = (DS.bf(nh * (1 + DS.TIE)) - DS.bf(nh * (1 - DS.TIE))).abs() * w.double().abs()          # a = bf16(x r) w may sit this far off
        rad = (da * cosd.abs() + DS.rotate_half(da).abs() * sind.abs()).reshape(b * heads, n, d) + NR_DEPTH * U24 * terms
        c = DS.bf(val)
        return c, torch.maximum((DS.bf(val + rad) - c).abs(), (DS.bf(val - rad) - c).abs())
    qc, dq_ = slack(t[0], qw, qv, tq)
    kc, dk_ = slack(t[1], kw, kv, tk)
    return qc.to(BF), kc.to(BF), v.to(BF), dq_, dk_


def nr_tables(n, d, seed):
    g = _gen(4242, n, d, seed)
    ang = torch.rand(n, d, generator=g) * 6.283
    return 1 + 0.2 * torch.randn(d, generator=g), 1 + 0.2 * torch.randn(d, generator=g), torch.cos(ang), torch.sin(ang)


# ---- emulations in kernel order: f32 where the kernels hold f32, bf16 where they round; `mutant` names one changed line (the negative controls) -----------------
def _f(t):
    return t.float()


def _bfr(t):
    return t.to(BF).float()


def emulate_forward(q, k, v, scale, mutant=None):
    """attention_kernel: raw scores, mask of the padded keys, row maximum, e = 2^(fma(s, ec, -m ec)), P V on the bf16 e, the f32 sum of the unrounded e -> (out bf16, lse f32)"""
    G, s, d = q.shape
    pad = nblocks(s) * 32
    sc = torch.zeros(G, s, pad)
    sc[..., :s] = _f(q) @ _f(k).transpose(-1, -2)                        # zero K rows past S: score 0
    live = torch.arange(pad) < s
    if mutant == "leak" and pad > s:
        live[s] = True                                                   # one padded key left unmasked
    if mutant == "mask_last":
        live[s - 1] = False                                              # the last live key masked
    sc = torch.where(live, sc, torch.full_like(sc, float("-inf")))
    if mutant == "half_max":                                             # the lower half-wave's keys only: key % 8 < 4
        m = torch.where((torch.arange(pad) % 8 < 4) & live, sc, torch.full_like(sc, float("-inf"))).max(-1, keepdim=True).values
    else:
        m = sc.max(-1, keepdim=True).values
    sf = torch.tensor(scale, dtype=F32)
    ec = sf * torch.tensor(LOG2E_F32, dtype=F32)
    emc = m * ec
    arg = (sc.double() * ec.double() - emc.double()).float()             # one rounding: the fma
    e = torch.exp2(arg)
    eb = _bfr(e)
    vp = torch.zeros(G, pad, d)
    vp[:, :s] = _f(v)
    tot = (eb if mutant == "sum_rounded" else e).sum(-1, keepdim=True)
    out = ((eb @ vp) * (1.0 / tot)).to(BF)
    lse = (m if mutant == "lse_noscale" else m * sf) + torch.log(tot)
    return out, lse.squeeze(-1)


def emulate_backward(q, k, v, o, do, scale, lse=None, mutant=None):
    """attention_bwd_lse*_kernel (lse given) or attention_bwd_kernel (lse None: its own max, sum and L) -> dq, dk, dv bf16"""
    sf = torch.tensor(scale, dtype=F32)
    l2e = torch.tensor(LOG2E_F32, dtype=F32)
    expf = lambda t: torch.exp2(t * l2e)                                 # __expf
    ob = _f(o)
    if mutant == "delta_other_head":
        ob = ob.roll(1, 0)
    delta = (_f(do) * ob).sum(-1, keepdim=True)
    xs = (_f(q) @ _f(k).transpose(-1, -2)) * sf
    dP = _f(do) @ _f(v).transpose(-1, -2)
    if lse is None:
        m = xs.max(-1, keepdim=True).values
        e = expf(xs - m)
        tot = e.sum(-1, keepdim=True)
        L = m + torch.log(tot)
        ds_a = e * ((1.0 / tot) * sf) * (dP - delta)                     # phase A: st * ps * (dpt - delta)
    else:
        L = lse.unsqueeze(-1)
        ds_a = None
    p = expf(xs - L)
    if mutant == "ds_round_first":
        ds = _bfr(p * (dP - delta)) * sf                                 # dS -> bf16 BEFORE the scale
    else:
        ds = p * (dP - delta) * sf
    ds_b = _bfr(ds)
    dq = (_bfr(ds_a) if ds_a is not None else ds_b) @ _f(k)
    dk = (_bfr(p * (dP - delta)) if mutant == "dk_noscale" else ds_b).transpose(-1, -2) @ _f(q)
    dv = _bfr(p).transpose(-1, -2) @ _f(do)
    return dq.to(BF), dk.to(BF), dv.to(BF)


def emulate_nr_operands(qkv, qw, kw, cos, sin, heads, eps):
    """dmvae_norm_rope8 in f32: r = rsqrt(ss / D + eps), bf16(x r) * w, the rotated pair, -> bf16 -> q, k, v [G, N, D] bf16"""
    b, n, c3 = qkv.shape
    d = c3 // 3 // heads
    t = qkv.float().view(b, n, 3, heads, d).permute(2, 0, 3, 1, 4)

    def one(u, w):
        r = torch.rsqrt((u * u).sum(-1, keepdim=True) / float(d) + torch.tensor(eps, dtype=F32))
        a = _bfr(u * r) * w.float()
        return (a * cos.float() + DS.rotate_half(a) * sin.float()).to(BF).reshape(b * heads, n, d)
    return one(t[0], qw), one(t[1], kw), t[2].to(BF).reshape(b * heads, n, d)


# ---- the many-block launch forms: which (sample, head) items to hold to fp64 ---------------------------------------------------------------------
def xcd_remap(flat, total):
    """common.h::xcd_remap"""
    qn, r, x = total >> 3, total & 7, flat & 7
    start = x * (qn + 1) if x < r else r * (qn + 1) + (x - r) * qn
    return start + (flat >> 3)


def spread_items(total):
    """>= 24 items: the first, the last, and of each of the eight remap classes (blocks flat = x mod 8) its first, middle and last block's item"""
    it = {0, total - 1}
    for x in range(8):
        n = (total - x + 7) // 8
        for i in (0, n // 2, n - 1):
            it.add(xcd_remap(x + 8 * i, total))
    extra = 1
    while len(it) < 24 and extra < total:
        it.add(extra)
        extra += total // 29 + 1
    return sorted(it)


# ==== the streaming kernels (csrc/attention_stream.hip, csrc/attention_bwd_stream.hip; any S) =========================================================================
# The same operation, so `reference` is the definition; the bars below are derived from THESE kernels' rounding sites (tests/test_attention_stream_spec_cpu.py,
# tests/test_gpu_attention_stream_spec.py).  nt = ceil(S / 64) key (query) tiles; t(j) = j // 64; xm_t = the running maximum of the scaled scores after tile t
# (xm_{nt-1} = xmax); u = 2^-8; one f32 rounding = 2^-24 of the value rounded.
#
# Forward (attention_stream_kernel).  The weight key j ends up with, in l and in the accumulators alike, is
#     w_j = 2^(fma(s_j, ec, -fl(m_t ec))) * alpha_{t+1} ... alpha_{nt-1},      alpha_v = 2^(fl(fl(m_{v-1} - m_v) ec)),   t = t(j)
# against exp(x_j - xmax); in exact arithmetic the exponents telescope.  Its relative error eps_s_j is the resident eps_j (scores E_x, ec's two roundings and the
# fma's one, v_exp_f32 at 1 ulp: the same instructions) plus what the tile walk adds:
#   emc_t     fl(m_t ec) is rounded per TILE (1 on |xm_t|): in the resident kernel it is common to the row and cancels in P; here keys of different tiles carry
#             different roundings, so it stays:                                                                   2^-24 |xm_t(j)|
#   alpha     for every later tile v: the difference (1) and its product with ec (1) on xm_v - xm_{v-1} -- summed over v that is the distance the maximum still
#             travels, 2 (xmax - xm_t(j)) --, the power (2: v_exp_f32) and the multiply `l *= alpha` / `o *= alpha` (1):    2^-24 (2 (xmax - xm_t(j)) + 3 (nt - 1 - t(j)))
#             (ec's own error multiplies the telescoped exponent x_j - xmax and is in eps_j already)
#       eps_s_j = eps_j + 2^-24 (|xm_t(j)| + 2 (xmax - xm_t(j)) + 3 (nt - 1 - t(j)))
#   row sum   the UNROUNDED p, 32 in-lane adds per tile and the half-wave sum at the end:     sum_depth = 32 nt + 1
#   P V       p -> bf16 once; 64 keys per tile into the f32 accumulators:                     pv_depth = 64 nt
#   lse       fl(fl(m scale) + __logf(l)): the resident expression on the streamed m and l:
#       E_lse = 2^-24 (4 |xmax| + sum_depth + 6 (lse - xmax) + |lse|) + sum_j p_j eps_s_j
#   out       o * (1 / l) -> bf16:
#       E_o = sum_j p_j (u + eps_s_j) |v_jd| + (sum_j p_j |v_jd|) (sum_j p_j eps_s_j + (pv_depth + sum_depth + 3) 2^-24)
# The mask of the ragged tile (score -inf, p = 0 exactly), the staging (copies) and the skipped waves round nothing.
#
# Backward (attention_bwd_stream_dq_kernel, attention_bwd_stream_dkdv_kernel); the sites its header lists, each against the resident derivation above:
#   q, k, v, dO, O bf16 operands       the same: no term
#   delta = dO . O, O as stored        the resident site (E_delta).  The order differs -- 8 KS in-lane fmas on exact products and one cross-half add, 33 / 41 roundings
#                                      -- and stays under the resident depth D + 1 = 65 / 73, which is kept.  |O - o| is `o_bar`: the forward's bar B_o when the
#                                      backward runs on the forward kernel's own out, u |o| when it runs on bf16(o) of the reference.
#                                      delta is written to caller memory by the query pass: an OUTPUT, held to E_delta; the key pass reads those bits back
#   scores, dP on the matrix cores     the same: E_x, E_dP with DP = 64 / 96 (five 16-channel steps at 72: under 96)
#   p = __expf(scale s - L) in f32     the resident site (eps_b) in BOTH passes, no running maximum: eps_b = eps_j + 3 * 2^-24 (lse - xmax) + E_L with E_L = the
#                                      forward's E_lse (its own lse) or 2^-24 |lse| (f32(lse) of the reference).  L and delta travel with a key-pass tile as f32
#                                      copies: no rounding; a padded query's L = +inf gives p = 0 exactly, a padded key's p is a select
#   P, scale dS -> bf16 once           the same (u; fl(fl(p (dP - delta)) scale): 4 * 2^-24).  Each pass rounds its own copy of the same f32 value
#   dQ, dK, dV f32 sums, bf16 once     DIFFERS in depth: the query pass adds 64 keys per tile over nt tiles into dQ, the key pass 64 queries per tile over nt tiles
#                                      into dK and dV: depth = 64 nt in both (resident: 32 nblk)
def _tile_of_key(s, dev):
    return torch.arange(s, device=dev) // STREAM_TILE


def bars_forward_stream(q, k, v, scale, ref):
    """-> dict o, lse (bounds on the bf16 out and the f32 lse) and the pieces bars_backward_stream reuses"""
    s, d = q.shape[-2:]
    dp, nt = staged(d), ntiles(s)
    qa, ka, va = q.double().abs(), k.double().abs(), v.double().abs()
    x, p, lse = ref["x"], ref["p"], ref["lse"]
    xmax = x.max(-1, keepdim=True).values
    e_x = dp * U24 * scale * qa @ ka.transpose(-1, -2)
    eps_res = U24 * (3 * x.abs() + 3 * (x - xmax).abs() + 2) + e_x                        # the resident eps_j
    tj = _tile_of_key(s, x.device)
    xm = torch.cummax(tile_max(x), -1).values[..., tj]                                    # xm_t(j) per (query, key)
    eps = eps_res + U24 * (xm.abs() + 2 * (xmax - xm) + 3 * (nt - 1 - tj).double())
    sum_depth, pv_depth = 32 * nt + 1, 64 * nt
    peps = (p * eps).sum(-1, keepdim=True)
    lsum = lse.unsqueeze(-1) - xmax
    e_lse = (U24 * (4 * xmax.abs() + sum_depth + 6 * lsum + lse.unsqueeze(-1).abs()) + peps).squeeze(-1)
    a = p @ va
    e_o = (p * (U8 + eps)) @ va + a * (peps + (pv_depth + sum_depth + 3) * U24) + TINY
    return dict(o=bf16_bound(ref["o"], e_o), lse=e_lse + TINY, eps_res=eps_res, xmax=xmax, e_lse=e_lse)


def bars_backward_stream(q, k, v, do, scale, ref, fwd, operands="kernel"):
    """-> dict dq, dk, dv (bf16) and delta (f32).  fwd = bars_forward_stream(...).  operands: "kernel" -- out / lse are the forward kernel's own, within fwd['o'] /
    fwd['lse'] of the definition; "reference" -- bf16(o) and f32(lse) of the definition"""
    s, d = q.shape[-2:]
    dp, nt = staged(d), ntiles(s)
    qa, ka, va, da = q.double().abs(), k.double().abs(), v.double().abs(), do.double().abs()
    p, lse = ref["p"], ref["lse"].unsqueeze(-1)
    if operands == "kernel":
        e_l, o_bar = fwd["e_lse"].unsqueeze(-1), fwd["o"]
    else:
        e_l, o_bar = U24 * lse.abs(), U8 * ref["o"].abs() + TINY
    eps_b = fwd["eps_res"] + 3 * U24 * (lse - fwd["xmax"]) + e_l
    depth = 64 * nt * U24
    e_dv = (p * (U8 + eps_b + depth)).transpose(-1, -2) @ da + TINY
    e_delta = (da * o_bar).sum(-1, keepdim=True) + (d + 1) * U24 * (da * ref["o"].abs()).sum(-1, keepdim=True)
    e_dp = dp * U24 * da @ va.transpose(-1, -2)
    t = scale * p * (ref["dP"] - ref["delta"]).abs()
    w = t * (U8 + eps_b + 4 * U24) + scale * p * (e_dp + e_delta) + depth * t
    return dict(dq=bf16_bound(ref["dq"], w @ ka + TINY), dk=bf16_bound(ref["dk"], w.transpose(-1, -2) @ qa + TINY), dv=bf16_bound(ref["dv"], e_dv),
                delta=e_delta.squeeze(-1) + TINY)


def reference_operands(ref):
    """the backward's saved operands made from the definition: bf16(o) [G, S, D], f32(lse) [G, S]"""
    return ref["o"].to(BF), ref["lse"].to(F32)


# ---- emulations in kernel order (CPU) -----------------------------------------------------------------------------------------------------------------------------------
_HALF_OF_KEY = (torch.arange(STREAM_TILE) % 8) // 4                    # the half-wave (lane >> 5) that holds a tile's key: register r of block kb is key
_LANE_ORDER = [[kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg for kb in range(2) for r in range(16)] for kg in range(2)]       # kb * 32 + (r & 3) + 8 (r >> 2) + 4 kg

FORWARD_STREAM_MUTANTS = ["leak", "alpha_o_only", "alpha_l_only", "alpha_sign", "half_max", "l_rounded", "lse_half", "stale_block"]
BACKWARD_STREAM_MUTANTS = ["skip_one_q", "skip_one_k", "kpass_256", "p_from_max", "delta_unrounded_o", "ds_round_first", "pad_cols"]


def emulate_forward_stream(q, k, v, scale, mutant=None):
    """attention_stream_kernel: per 64-key tile the raw scores, the mask of the ragged tile, the running maximum (per half-wave, exchanged), alpha, `l *= alpha`,
    `o *= alpha`, p = 2^(fma(s, ec, -m ec)), l += p in the lane's register order, P V on the bf16 p in four 16-key steps; then the half-wave sum, o * (1 / l) and
    lse = m scale + log(l) -> (out bf16, lse f32, dict o32 = the unrounded o * (1 / l), m = the final raw maximum).
    State is kept per half-wave (m, l: [G, S, 2]; a channel c of the accumulators sits in half (c % 8) // 4), which is what lets the mutants be one changed line."""
    G, s, d = q.shape
    nt = ntiles(s)
    pad = nt * STREAM_TILE
    qf = _f(q)
    kp, vp = torch.zeros(G, pad, d), torch.zeros(G, pad, d)             # rows past S are staged as zeros
    kp[:, :s], vp[:, :s] = _f(k), _f(v)
    sf = torch.tensor(scale, dtype=F32)
    ec = sf * torch.tensor(LOG2E_F32, dtype=F32)
    chalf = (torch.arange(d) % 8) // 4
    ninf = torch.tensor(float("-inf"))
    m, l, o = torch.full((G, s, 2), float("-inf")), torch.zeros(G, s, 2), torch.zeros(G, s, d)
    for t in range(nt):
        kt, vt = kp[:, t * 64:t * 64 + 64], vp[:, t * 64:t * 64 + 64]
        if mutant == "stale_block" and t > 0:                           # the tile's second block read from the other buffer: tile t - 1's image
            kt, vt = torch.cat([kt[:, :32], kp[:, t * 64 - 32:t * 64]], 1), torch.cat([vt[:, :32], vp[:, t * 64 - 32:t * 64]], 1)
        sc = qf @ kt.transpose(-1, -2)
        lim = s - t * 64
        if mutant == "leak" and lim < 64:
            lim += 1                                                    # one padded key of the last tile left unmasked
        sc = torch.where(torch.arange(64) < lim, sc, ninf)
        tmh = torch.stack([sc[..., _HALF_OF_KEY == hh].max(-1).values for hh in range(2)], -1)
        tm = tmh if mutant == "half_max" else tmh.max(-1, keepdim=True).values.expand(-1, -1, 2)      # xhalf_max
        mn = torch.maximum(m, tm)
        if mutant == "alpha_sign":
            alpha = torch.where(torch.isinf(m), torch.zeros(()), torch.exp2((mn - m) * ec))
        else:
            alpha = torch.exp2((m - mn) * ec)                           # first tile: 2^(-inf) = 0
        emc = mn * ec
        m = mn
        if mutant != "alpha_o_only":
            l = l * alpha
        if mutant != "alpha_l_only":
            o = o * alpha[..., chalf]
        e = torch.exp2((sc.double() * ec.double() - emc[..., _HALF_OF_KEY].double()).float())        # one rounding: the fma
        eb = _bfr(e)
        ea = eb if mutant == "l_rounded" else e
        lh = []
        for hh in range(2):
            acc = l[..., hh]
            for j in _LANE_ORDER[hh]:
                acc = acc + ea[..., j]
            lh.append(acc)
        l = torch.stack(lh, -1)
        for c in range(0, 64, 16):
            o = o + eb[..., c:c + 16] @ vt[:, c:c + 16]
    lt = l[..., 0] + l[..., 1]                                          # xhalf_sum
    o32 = o * (1.0 / lt).unsqueeze(-1)
    lse = m[..., 0] * sf + torch.log(l[..., 0] if mutant == "lse_half" else lt)
    return o32.to(BF), lse, dict(o32=o32, m=m[..., 0])


def emulate_backward_stream(q, k, v, o, do, lse, scale, rows=None, mutant=None, o32=None, m=None):
    """the two passes -> dq, dk [G, S, rows or D] bf16, dv [G, S, D] bf16, delta [G, S] f32.  delta: per half-wave the in-lane chain over its 8-channel pieces, then
    the cross-half add.  Both passes rebuild p = __expf(s scale - L) and dS = fl(fl(p (dP - delta)) scale) in f32 and round their own bf16 copy; the query pass adds
    dS K over the key tiles in 16-key steps, the key pass P^T dO and dS^T Q over the query tiles in 16-query steps.  o32, m: the forward emulation's extras, for
    the mutants that take the unrounded O or the running maximum."""
    G, s, d = q.shape
    nt, ks = ntiles(s), (4 if d == 64 else 5)
    sf = torch.tensor(scale, dtype=F32)
    l2e = torch.tensor(LOG2E_F32, dtype=F32)
    qf, kf, vf, dof = _f(q), _f(k), _f(v), _f(do)
    prod = dof * (o32 if mutant == "delta_unrounded_o" else _f(o))
    dh = []
    for hh in range(2):
        acc = torch.zeros(G, s)
        for kk in range(ks):
            for c in range(kk * 16 + hh * 8, min(kk * 16 + hh * 8 + 8, d)):
                acc = acc + prod[..., c]
        dh.append(acc)
    delta = (dh[0] + dh[1]).unsqueeze(-1)
    xs = (qf @ kf.transpose(-1, -2)) * sf
    dP = dof @ vf.transpose(-1, -2)
    L = (m * sf if mutant == "p_from_max" else lse).unsqueeze(-1)
    p = torch.exp2((xs - L) * l2e)                                      # __expf
    if mutant == "ds_round_first":
        ds_b = _bfr(_bfr(p * (dP - delta)) * sf)                        # dS -> bf16 BEFORE the scale
    else:
        ds_b = _bfr(p * (dP - delta) * sf)
    pb = _bfr(p)
    one_left = s - (nt - 1) * 64 == 33                                  # the last tile's second block holds exactly one live row
    nq = s - 1 if mutant == "skip_one_q" and one_left else s            # keys the query pass walks
    nk = s - 1 if mutant == "skip_one_k" and one_left else s            # queries the key pass walks
    dq, dk, dv = torch.zeros(G, s, d), torch.zeros(G, s, d), torch.zeros(G, s, d)
    for c in range(0, nq, 16):
        e = min(c + 16, nq)
        dq = dq + ds_b[..., c:e] @ kf[:, c:e]
    for c in range(0, nk, 16):
        e = min(c + 16, nk)
        dv = dv + pb[:, c:e].transpose(-1, -2) @ dof[:, c:e]
        dk = dk + ds_b[:, c:e].transpose(-1, -2) @ qf[:, c:e]
    if mutant == "kpass_256" and d == 72:                               # four waves = 128 keys per workgroup on a grid of ceil(S / 256): keys 128 .. 255 of each
        dead = (torch.arange(s) % 256) >= 128                           # 256 are nobody's, the caller's pre-fill stays
        dk[:, dead], dv[:, dead] = float("nan"), float("nan")
    dq, dk = dq.to(BF), dk.to(BF)
    if rows is not None and rows > d:
        dq, dk = pad_rows(dq, rows), pad_rows(dk, rows)
        if mutant == "pad_cols":                                        # the products over the padded channels taken on what is not zero
            dq[..., d:], dk[..., d:] = dq[..., :rows - d], dk[..., :rows - d]
    return dq, dk, dv.to(BF), delta.squeeze(-1)


def padded_columns_are_zero(t, d):
    return t.shape[-1] == d or float(t[..., d:].float().abs().max()) == 0.0


# ==== the d = 512 streaming kernels (csrc/attention_wide.hip, csrc/attention_wide_bwd.hip; one head, any S) ===========================================================
# The same operation, so `reference` is the definition; cases are make_case(kind, b, 1, s, 512, tile=32).  The bars below are derived from THESE kernels' rounding sites
# (tests/test_attention_wide_spec_cpu.py, tests/test_gpu_attention_wide_spec.py).  nt = ceil(S / 32) key (row) tiles; t(j) = j // 32; xm_t = the running maximum of the
# scaled scores after tile t; u = 2^-8; one f32 rounding = 2^-24 of the value rounded.
#
# Forward (attention_wide_kernel).  Two waves share 32 queries and run the same score and softmax instructions on the same data, each on its half of the output
# channels: the sites are per (query, key) and per (query, channel) as in the streaming kernel, with other depths.
#   scores    st accumulates KS = 32 sixteen-channel MFMA steps: an f32 sum of 512 exact products:        E_x = 512 2^-24 scale sum_d |q_d k_d|
#   power     2^(fma(st, ec, -emc)), ec = fl(scale fl(log2 e)), v_exp_f32: the resident figure             eps_j = 2^-24 (3 |x_j| + 3 |x_j - xmax| + 2) + E_x_j
#   emc       fl(mn ec) once per 32-key TILE (1 on |xm_t|): keys of different tiles carry different roundings: 2^-24 |xm_t(j)|
#   alpha     2^(fl(fl(m - mn) ec)) for every later tile v: the difference and the product (2 on xm_v - xm_{v-1}; summed over v: 2 (xmax - xm_t(j))), the power (2) and
#             the multiply `l *= alpha` / `o[db][r] *= alpha` (1):                                         2^-24 (2 (xmax - xm_t(j)) + 3 (nt - 1 - t(j)))
#       eps_w_j = eps_j + 2^-24 (|xm_t(j)| + 2 (xmax - xm_t(j)) + 3 (nt - 1 - t(j)))
#   row sum   `l += st[r]` on the UNROUNDED p: 16 in-lane adds per tile (a lane holds 16 of the tile's 32 keys), xhalf_sum at the end:    sum_depth = 16 nt + 1
#   P V       to_afrag rounds p to bf16 once (u); two 16-key MFMA steps per tile into the f32 accumulators:                              pv_depth = 32 nt
#   lse       fl(fl(m scale) + __logf(l)), the streaming expression:   E_lse = 2^-24 (4 |xmax| + sum_depth + 6 (lse - xmax) + |lse|) + sum_j p_j eps_w_j
#   out       inv = 1 / l (1), o * inv (1), the accumulators' own rounding into bf16 is bf16_bound's; the 3 of the streaming form is kept:
#       E_o = sum_j p_j (u + eps_w_j) |v_jd| + (sum_j p_j |v_jd|) (sum_j p_j eps_w_j + (pv_depth + sum_depth + 3) 2^-24)
# The half-wave mask of the ragged tile (score -inf, p = 0 exactly), the staging, the idle wave pair and the choice of the lane that writes lse round nothing.
#
# Backward (attention_wide_bwd_dq_kernel, attention_wide_bwd_dkdv_kernel).  Both passes form the same f32 values (the same instructions on the same operands, the
# key on the lane or the query on the lane), so one set of sites:
#   scores, dP   per wave KS = 8 sixteen-channel steps over ITS 128 channels (128 2^-24 of that quarter's magnitudes), then xch_sum's three f32 adds ((0 + 1) + 2) + 3,
#                each 2^-24 of a partial sum no larger than the whole magnitude sum:  E_xb = 131 2^-24 scale sum_d |q_d k_d|,  E_dP = 131 2^-24 sum_d |dO_qd v_jd|
#   p            __expf(fl(st scale) - L) (or the contracted fma: one rounding fewer): the product (1 on |x|), the difference and the product with fl(log2 e)
#                (3 on |x - L| <= |x - xmax| + (lse - xmax)), v_exp_f32 (2); L is the caller's f32 lse, off by E_L = the wide forward's E_lse (its own lse) or
#                2^-24 |lse| (f32(lse) of the definition):       eps_b = 2^-24 (3 |x| + 3 |x - xmax| + 2) + E_xb + 3 * 2^-24 (lse - xmax) + E_L
#   delta        sum_k p dP by fmaf over the kernel's OWN p and dP -- `o` is not read, there is no dO . O and no term of the stored O's rounding: a lane chains its 16
#                keys of every tile (16 nt fmas), xhalf_sum adds the two halves (1).  An OUTPUT in caller memory; the key pass reads those bits back:
#                    E_delta = sum_j p_j (eps_b_j |dP_j| + E_dP_j) + (16 nt + 1) 2^-24 sum_j p_j |dP_j|
#   scale dS     x = fl(fl(p fl(dP - delta)) scale): three roundings on T = scale p |dP - delta|; p's eps_b on T; E_dP + E_delta on the difference.  x enters the
#                matrix cores as hi + lo, hi = bf16(x), lo = bf16(x - hi): x - hi is exact in f32 and at most u |x|, so what is lost is at most u^2 |x| = 2^-16 |x|
#                (the header's 2^-17-class figure with u as half an ulp of 2^-9; the sibling's single bf16 loses u |x|):
#                    W_qj = T_qj (u^2 + eps_b + 3 * 2^-24) + scale p_qj (E_dP + E_delta)
#   dQ, dK       per 32-row tile two 16-row steps, each a product on hi and one on lo into the same f32 accumulator: 64 nt summands, the lo half of them u times smaller:
#                    E_dq = sum_j (W_qj + 64 nt (1 + u) 2^-24 T_qj) |k_jd|;  E_dk the same over the queries with |q_qd|
#   dV           P -> bf16 once (u), two 16-query steps per tile: E_dv = sum_q p_qj (u + eps_b + 32 nt 2^-24) |dO_qd|
# Padded rows round nothing: zero staging, the select (query pass), L = +inf (key pass).
WIDE_QUARTER_DEPTH = WIDE_D // 4 + 3          # 128 products of a wave's quarter, three adds across the quarters


def wide_ntiles(s):
    return ntiles(s, WIDE_TILE)


def make_wide_case(kind, s, b=1, seed=0):
    return make_case(kind, b, 1, s, WIDE_D, seed=seed, tile=WIDE_TILE)


def bars_forward_wide(q, k, v, scale, ref):
    """-> dict o, lse (bounds on the bf16 out and the f32 lse) and the pieces bars_backward_wide reuses"""
    s, d = q.shape[-2:]
    nt = wide_ntiles(s)
    qa, ka, va = q.double().abs(), k.double().abs(), v.double().abs()
    x, p, lse = ref["x"], ref["p"], ref["lse"]
    xmax = x.max(-1, keepdim=True).values
    qk = scale * qa @ ka.transpose(-1, -2)
    site = U24 * (3 * x.abs() + 3 * (x - xmax).abs() + 2)                                  # the power, without the scores' own term
    tj = torch.arange(s, device=x.device) // WIDE_TILE
    xm = torch.cummax(tile_max(x, WIDE_TILE), -1).values[..., tj]                          # xm_t(j) per (query, key)
    eps = site + d * U24 * qk + U24 * (xm.abs() + 2 * (xmax - xm) + 3 * (nt - 1 - tj).double())
    sum_depth, pv_depth = 16 * nt + 1, 32 * nt
    peps = (p * eps).sum(-1, keepdim=True)
    lsum = lse.unsqueeze(-1) - xmax
    e_lse = (U24 * (4 * xmax.abs() + sum_depth + 6 * lsum + lse.unsqueeze(-1).abs()) + peps).squeeze(-1)
    a = p @ va
    e_o = (p * (U8 + eps)) @ va + a * (peps + (pv_depth + sum_depth + 3) * U24) + TINY
    return dict(o=bf16_bound(ref["o"], e_o), lse=e_lse + TINY, site=site, qk=qk, xmax=xmax, e_lse=e_lse)


def bars_backward_wide(q, k, v, do, scale, ref, fwd, operands="kernel"):
    """-> dict dq, dk, dv (bf16) and delta (f32).  fwd = bars_forward_wide(...).  operands: "kernel" -- lse is the wide forward's own, within fwd['lse'] of the
    definition; "reference" -- f32(lse) of the definition.  (`o` is not an operand: the kernel does not read it.)"""
    s, d = q.shape[-2:]
    nt = wide_ntiles(s)
    qa, ka, va, da = q.double().abs(), k.double().abs(), v.double().abs(), do.double().abs()
    p, lse = ref["p"], ref["lse"].unsqueeze(-1)
    e_l = fwd["e_lse"].unsqueeze(-1) if operands == "kernel" else U24 * lse.abs()
    eps_b = fwd["site"] + WIDE_QUARTER_DEPTH * U24 * fwd["qk"] + 3 * U24 * (lse - fwd["xmax"]) + e_l
    e_dp = WIDE_QUARTER_DEPTH * U24 * da @ va.transpose(-1, -2)
    dpa = ref["dP"].abs()
    e_delta = (p * (eps_b * dpa + e_dp)).sum(-1, keepdim=True) + (16 * nt + 1) * U24 * (p * dpa).sum(-1, keepdim=True)
    t = scale * p * (ref["dP"] - ref["delta"]).abs()
    w = t * (U8 * U8 + eps_b + 3 * U24) + scale * p * (e_dp + e_delta) + 64 * nt * (1 + U8) * U24 * t
    e_dv = (p * (U8 + eps_b + 32 * nt * U24)).transpose(-1, -2) @ da + TINY
    return dict(dq=bf16_bound(ref["dq"], w @ ka + TINY), dk=bf16_bound(ref["dk"], w.transpose(-1, -2) @ qa + TINY), dv=bf16_bound(ref["dv"], e_dv),
                delta=e_delta.squeeze(-1) + TINY)


# ---- emulations in kernel order (CPU) -----------------------------------------------------------------------------------------------------------------------------------
_W_HALF = (torch.arange(WIDE_TILE) % 8) // 4                           # the half-wave (kg = lane >> 5) that holds a tile's key: register r is key (r & 3) + 8 (r >> 2) + 4 kg
_W_LANE_ORDER = [[(r & 3) + 8 * (r >> 2) + 4 * kg for r in range(16)] for kg in range(2)]

FORWARD_WIDE_MUTANTS = ["leak", "mask_ignores_half", "alpha_o_only", "alpha_l_only", "half_max", "lse_half", "l_rounded", "stale_tile"]
BACKWARD_WIDE_MUTANTS = ["delta_from_O", "ds_single_bf16", "quarter_dropped", "p_from_max", "dk_noscale", "skip_one_q", "skip_one_k", "pad_key_unselected",
                         "pad_query_finite_L"]


def emulate_forward_wide(q, k, v, scale, mutant=None):
    """attention_wide_kernel: per 32-key tile the raw scores, the half-wave mask of the ragged tile (register index < lim = S - 32 t - 4 kg), the running maximum (per
    half-wave, exchanged), alpha, `l *= alpha`, `o *= alpha`, p = 2^(fma(s, ec, -m ec)), l += p in the lane's register order, P V on the bf16 p in two 16-key steps;
    then the half-wave sum, o * (1 / l) and lse = m scale + log(l) -> (out bf16, lse f32, dict m = the final raw maximum).  State per half-wave (m, l: [G, S, 2];
    channel c of the accumulators sits in half (c % 8) // 4: registers 4 r4 .. 4 r4 + 3 are channels 32 db + 8 r4 + 4 kg + 0 .. 3)."""
    G, s, d = q.shape
    nt = wide_ntiles(s)
    pad = nt * WIDE_TILE
    kp, vp = torch.zeros(G, pad, d), torch.zeros(G, pad, d)             # rows past S are staged as zeros
    kp[:, :s], vp[:, :s] = _f(k), _f(v)
    raw = _f(q) @ kp.transpose(-1, -2)
    sf = torch.tensor(scale, dtype=F32)
    ec = sf * torch.tensor(LOG2E_F32, dtype=F32)
    chalf = (torch.arange(d) % 8) // 4
    ninf = torch.tensor(float("-inf"))
    idx = torch.arange(WIDE_TILE) - 4 * _W_HALF                         # (r & 3) + 8 (r >> 2) of the register that holds the key
    m, l, o = torch.full((G, s, 2), float("-inf")), torch.zeros(G, s, 2), torch.zeros(G, s, d)
    for t in range(nt):
        tt = t - 1 if mutant == "stale_tile" and t > 0 else t          # the K / V image of tile t - 1: the other buffer
        sc, vt = raw[..., tt * 32:tt * 32 + 32], vp[:, tt * 32:tt * 32 + 32]
        if t * 32 + 32 > s:                                             # the last tile of a ragged S
            lim = s - t * 32 + (1 if mutant == "leak" else 0)           # leak: one padded key left unmasked
            sc = torch.where(idx < lim - (0 if mutant == "mask_ignores_half" else 4 * _W_HALF), sc, ninf)
        tmh = torch.stack([sc[..., _W_HALF == hh].max(-1).values for hh in range(2)], -1)
        tm = tmh if mutant == "half_max" else tmh.max(-1, keepdim=True).values.expand(-1, -1, 2)      # xhalf_max
        mn = torch.maximum(m, tm)
        alpha = torch.exp2((m - mn) * ec)                               # first tile: 2^(-inf) = 0
        emc = mn * ec
        m = mn
        if mutant != "alpha_o_only":
            l = l * alpha
        if mutant != "alpha_l_only":
            o = o * alpha[..., chalf]
        e = torch.exp2((sc.double() * ec.double() - emc[..., _W_HALF].double()).float())            # one rounding: the fma
        eb = _bfr(e)
        ea = eb if mutant == "l_rounded" else e
        lh = []
        for hh in range(2):
            acc = l[..., hh]
            for j in _W_LANE_ORDER[hh]:
                acc = acc + ea[..., j]
            lh.append(acc)
        l = torch.stack(lh, -1)
        for c in (0, 16):
            o = o + eb[..., c:c + 16] @ vt[:, c:c + 16]
    lt = l[..., 0] + l[..., 1]                                          # xhalf_sum
    o32 = o * (1.0 / lt).unsqueeze(-1)
    lse = m[..., 0] * sf + torch.log(l[..., 0] if mutant == "lse_half" else lt)
    return o32.to(BF), lse, dict(m=m[..., 0])


def emulate_backward_wide(q, k, v, o, do, lse, scale, mutant=None, m=None):
    """the two passes on rows padded to whole 32-row tiles, as staged (zero rows) -> dq, dk, dv [G, S, 512] bf16, delta [G, S] f32.  Scores and dP: per 128-channel
    quarter, the quarters added ((0 + 1) + 2) + 3.  p = __expf(s scale - L): a padded query has L = +inf in both passes, a padded key is a select in the query pass
    (the key pass does not store its padded keys).  First walk: delta by fmaf down the lane's 16 keys of every tile, per half-wave, then the cross-half add.  Second
    walk and key pass: x = fl(fl(p (dP - delta)) scale), hi = bf16(x), lo = bf16(x - hi); dQ += hi K, += lo K per 16-key step; dV += P^T dO, dK += hi^T Q, += lo^T Q
    per 16-query step.  `o` is used by the mutant delta_from_O alone, `m` (the forward emulation's final raw maximum) by p_from_max."""
    G, s, d = q.shape
    nt = wide_ntiles(s)
    pad = nt * WIDE_TILE
    sf = torch.tensor(scale, dtype=F32)
    l2e = torch.tensor(LOG2E_F32, dtype=F32)

    def rows(t):
        z = torch.zeros(G, pad, d)
        z[:, :s] = _f(t)
        return z
    qf, kf, vf, dof = rows(q), rows(k), rows(v), rows(do)
    nquart = 3 if mutant == "quarter_dropped" else 4

    def quarters(a, b):
        part = [a[..., w * 128:w * 128 + 128] @ b[..., w * 128:w * 128 + 128].transpose(-1, -2) for w in range(nquart)]
        acc = part[0]
        for w in range(1, nquart):
            acc = acc + part[w]
        return acc
    xs = quarters(qf, kf) * sf
    dP = quarters(dof, vf)
    live = torch.arange(pad) < s
    L = torch.full((G, pad), float("inf"))
    L[:, :s] = m * sf if mutant == "p_from_max" else lse
    p = torch.exp2((xs - L.unsqueeze(-1)) * l2e)                        # __expf; rows of padded queries are 0
    # ---- query pass ----
    nq = s - 1 if mutant == "skip_one_q" and s % 32 == 1 else pad       # keys the query pass walks: the single live key of the last tile not walked
    pq = p if mutant == "pad_key_unselected" else torch.where(live, p, torch.zeros(()))
    if mutant == "delta_from_O":                                        # the sibling kernel's site: dO . O on the stored bf16 O
        delta = torch.zeros(G, pad)
        delta[:, :s] = (_f(do) * _f(o)).sum(-1)
    else:
        dh = []
        for hh in range(2):
            acc = torch.zeros(G, pad, dtype=D64)
            for t in range((nq + 31) // 32):
                for j in _W_LANE_ORDER[hh]:
                    if t * 32 + j < nq:
                        acc = (pq[..., t * 32 + j].double() * dP[..., t * 32 + j].double() + acc).float().double()      # fmaf
            dh.append(acc.float())
        delta = dh[0] + dh[1]                                           # xhalf_sum

    def hi_lo(pp, dl, unscaled=False):
        x = pp * (dP - dl.unsqueeze(-1))
        x = x if unscaled else x * sf
        hi = _bfr(x)
        return hi, (torch.zeros_like(hi) if mutant == "ds_single_bf16" else _bfr(x - hi))
    hi, lo = hi_lo(pq, delta)
    dq = torch.zeros(G, pad, d)
    for c in range(0, nq, 16):
        e = min(c + 16, nq)
        dq = dq + hi[..., c:e] @ kf[:, c:e]
        dq = dq + lo[..., c:e] @ kf[:, c:e]
    # ---- key pass: L and delta of a tile's queries travel with it; the delta bits are the query pass's ----
    pk, dk_delta = p, delta.clone()
    if mutant == "pad_query_finite_L" and pad > s:                      # the unselected loads of row S - 1
        Lk = L.clone()
        Lk[:, s:], dk_delta[:, s:] = L[:, s - 1:s], delta[:, s - 1:s]
        pk = torch.exp2((xs - Lk.unsqueeze(-1)) * l2e)
    nk = s - 1 if mutant == "skip_one_k" and s % 32 == 1 else pad       # queries the key pass walks
    hk, lk = hi_lo(pk, dk_delta, unscaled=mutant == "dk_noscale")
    pb = _bfr(pk)
    dk, dv = torch.zeros(G, pad, d), torch.zeros(G, pad, d)
    for c in range(0, nk, 16):
        e = min(c + 16, nk)
        dv = dv + pb[:, c:e].transpose(-1, -2) @ dof[:, c:e]
        dk = dk + hk[:, c:e].transpose(-1, -2) @ qf[:, c:e]
        dk = dk + lk[:, c:e].transpose(-1, -2) @ qf[:, c:e]
    return dq[:, :s].to(BF), dk[:, :s].to(BF), dv[:, :s].to(BF), delta[:, :s].contiguous()
