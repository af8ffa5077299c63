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
dq 0.334, dk 0.388, dv 0.876; NR out 0.574.  No bar needed widening; the negative controls and what each reaches are listed in that module's docstring."""
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


def classes_at(s):
    return CLASSES if s in ALL_CLASS_TOKENS else CLASSES[:2]


def staged(d):
    return (d + 31) // 32 * 32


def nblocks(s):
    return (s + 31) // 32


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


def make_case(kind, b, h, s, d, seed=0):
    """-> dict of q, k, v, do [G, S, D] bf16 on the CPU, scale = d ** -0.5.  Classes (u: one unit direction per item, r = sqrt(d) / 8 so that scores are those of d = 64):
    randn (x 1.5), randn4 (x 4: peaked rows);
    negative  q = -g u, k = c u, g in [14, 16], c in sqrt(d) [0.62, 1] (d = 64: [4.96, 8]): every scaled score in [-16, -8.6] -- a key left at score 0 takes the weight
              (with a unit u, c below 4.6 would put scores above -8 and the class's own assertion would fail);
    last      q = g u, k = 0.2 linspace(0, 8) r u but the last key 8 r u: the last key takes >= 0.99 of every row (the only live key of its block at S = 32 k + 1);
    zeroq     zero queries: uniform rows, o = mean V, lse = log S;
    offset    k = a u + 0.1 randn, q = +- a u + 0.5 randn with scale a^2 = 80: |lse| ~ 80, where an f32 ulp is 8e-6;
    spike     keys 0.05 r u but key spike_key(S) = 56 r u, q = g u: that key scores ~105 against < 1, so a row maximum that misses it overflows the power."""
    g = _gen(CLASSES.index(kind), b, h, s, d, seed)
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
    else:
        raise ValueError(kind)
    return dict(kind=kind, b=b, h=h, s=s, d=d, scale=d ** -0.5, q=q.to(BF), k=k.to(BF), v=v.to(BF), do=rn(G, s, d).to(BF))


def check_class(c, ref):
    """the assertion ON THE REFERENCE ALONE that a class does what it is for"""
    kind, s = c["kind"], c["s"]
    x = ref["x"]
    if kind == "negative":
        assert float(x.max()) <= -8.0, float(x.max())
    elif kind == "last":
        assert float(ref["p"][..., -1].min()) >= 0.99, float(ref["p"][..., -1].min())
    elif kind == "zeroq":
        assert float((ref["o"] - c["v"].double().mean(1, keepdim=True)).abs().max()) < 1e-12 and float((ref["lse"] - math.log(s)).abs().max()) < 1e-12
    elif kind == "offset":
        assert float(ref["lse"].abs().min()) >= 60.0, float(ref["lse"].abs().min())
    elif kind == "spike" and s > 1:
        j = spike_key(s)
        rest = torch.cat([x[..., :j], x[..., j + 1:]], -1)
        assert float((x[..., j] - rest.max(-1).values).min()) >= 96.0      # > log(FLT_MAX) = 88.7
        assert float(ref["p"][..., j].min()) >= 1 - 1e-30


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
