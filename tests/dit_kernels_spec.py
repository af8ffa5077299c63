"""Not a test: the fp64 restatement of the LightningDiT elementwise kernels (csrc/dit.hip), the element-wise bars their outputs are held to, and the inputs
the tests share (tests/test_dit_kernels_spec_cpu.py, tests/test_gpu_dit_forms.py, tests/test_gpu_dit.py).  Nothing here needs a GPU or imports dmvae_amd.

Definitions: plain torch in float64 from the header comment of dit.hip, rounding to bf16 (`bf`, ties to even, on the fp64 value itself) exactly at the sites the
comment names -- bf16(1 + scale), bf16(q * rq) before the norm weight, bf16(silu), bf16(gate * y) -- with the gradient passed straight through a rounding.

Bars (`check_bf16`, `check_f32`, `check_bf16_sites`): every element at its own magnitude.
  * A bf16 output is compared with the UNROUNDED fp64 value of its last expression; that rounding contributes a half-ulp, at most 2^-8 of the value.
  * A rounding site INSIDE the expression whose operand is exact in the kernel (1 + scale: a bf16 plus one, exact in f32 and f64 alike above 2^-16, and below
    it both round to 1) is applied in the reference and contributes nothing.
  * A site whose operand carries the kernel's f32 error (silu through exp and rcp, q * rq through the sum and rsqrt) can round to the other neighbour next to a
    tie.  The reference leaves such a site unrounded and the bound takes a half-ulp of every term the rounding propagates through (the sum over k of |t_k|);
    `check_bf16_sites` in addition holds the output to ONE final rounding of a product whose rounded factor is any bf16 value the site can legitimately give.
  * f32 work before the last rounding: depth * 2^-24 * sum |terms|, depth = the number of f32 roundings on the longest path, counted from the kernel's loops by
    the depth functions below (no fitted constant anywhere).
Measured on the f32 CPU emulations of tests/test_dit_kernels_spec_cpu.py (the only arbiter the bars have): worst |error| / bound over its cases 0.99 for the
bf16 bars (the half-ulp at the bottom of a binade, under the factor 1.01) and 0.30 (dgate), 0.21 (dscale), 0.12 (dx, dshift, dq_weight), 0.04 (dw) for the f32
bars; no bar needed widening."""
import torch
import torch.nn.functional as F

BF = torch.bfloat16
U8 = 2.0 ** -8          # half an ulp of bf16 relative to the value, at most (8 significand bits)
U24 = 2.0 ** -24        # one f32 rounding, relative
EPS = 1e-6


def bf(x: torch.Tensor) -> torch.Tensor:
    """fp64 -> the nearest bf16 value (ties to even) as fp64, rounded from the fp64 value directly (no intermediate f32); normal range only."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def ste(x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """value r, gradient of x"""
    return x + (r - x).detach()


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    p = x.reshape(*x.shape[:-1], -1, 2)
    return torch.stack((-p[..., 1], p[..., 0]), dim=-1).reshape(x.shape)


def rotate_half_t(x: torch.Tensor) -> torch.Tensor:
    """the transpose of rotate_half"""
    p = x.reshape(*x.shape[:-1], -1, 2)
    return torch.stack((p[..., 1], -p[..., 0]), dim=-1).reshape(x.shape)


# ---- definitions ----------------------------------------------------------------------------------------------------------------------
def rmsnorm_modulate(x, w, scale, shift=None, eps=EPS, rnd=True):
    """x [B,N,C], w [C], scale / shift [B,C] -> (value [B,N,C] before its bf16 rounding, terms = |nrm * m| + |shift|)."""
    x, w, scale = x.double(), w.double(), scale.double()
    nrm = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
    m = 1 + scale
    if rnd:
        m = ste(m, bf(m))
    t = nrm * m.unsqueeze(1)
    if shift is None:
        return t, t.abs()
    sh = shift.double().unsqueeze(1)
    return t + sh, t.abs() + sh.abs()


def gated_residual_f64(x, gate, y, rnd=True):
    """x [B,N,C] + bf16(gate[b] * y) in fp64 (the differentiable definition)."""
    p = gate.double().unsqueeze(1) * y.double()
    return x.double() + (ste(p, bf(p)) if rnd else p)


def gated_residual_exact(x, gate, y):
    """The f32 residual stream bit for bit: a product of two bf16 values is exact in f32, one rounding to bf16, one f32 addition."""
    return x + (gate.float().unsqueeze(1) * y.float()).to(BF).float()


def gated_residual_bwd(dx, gate, y):
    """-> (dy bf16, bit-exact: one f32 product, one rounding; dgate [B,C] fp64; its terms)."""
    dy = (gate.float().unsqueeze(1) * dx).to(BF)
    p = dx.double() * y.double()
    return dy, p.sum(1), p.abs().sum(1)


def swiglu(x12, rnd=True):
    """[x1 | x2] -> (silu(x1) * x2 with the gate rounded or not, the unrounded gate s)."""
    x = x12.double()
    hid = x.shape[-1] // 2
    s = F.silu(x[..., :hid])
    return (ste(s, bf(s)) if rnd else s) * x[..., hid:], s


def silu_err(x1):
    """Relative f32 error of the kernels' x * rcp(1 + exp(-x)): the exponent x * log2(e) is rounded once (|x| 2^-24 relative on the power), exp2, the add, the
    reciprocal and the product one rounding each -> (|x| + 4.5) 2^-24; taken as (1.5 |x| + 8) 2^-24."""
    return (1.5 * x1.double().abs() + 8.0) * U24


def swiglu_bwd(dh, x12):
    """-> (dx12 value before its rounding [rows, 2 hid], f32 terms of the same shape, the unrounded gate s)."""
    x = x12.double()
    hid = x.shape[-1] // 2
    x1, x2, d = x[..., :hid], x[..., hid:], dh.double()
    sg = torch.sigmoid(x1)
    s = x1 * sg
    g1 = d * x2 * sg * (1 + x1 * (1 - sg))
    t1 = (d * x2).abs() * sg * (1 + 2 * x1.abs())         # |dh x2| s (1 + |x| (1 - s)) and the error of 1 - s carried through x
    return torch.cat([g1, d * bf(s)], -1), torch.cat([t1, (d * s).abs()], -1), s


def _heads(qkv, heads):
    b, n, c3 = qkv.shape
    d = c3 // 3 // heads
    return qkv.double().view(b, n, 3, heads, d).permute(2, 0, 3, 1, 4), d     # [3][B][H][N][D]


def qknorm_rope(qkv, qw, kw, cos, sin, heads, eps=EPS, rnd=True):
    """qkv [B,N,3 H D], cos / sin [N,D] independent tables -> (q, k values [B*H,N,D] before their rounding, their terms |a cos| + |rot(a) sin|, v exact)."""
    t, d = _heads(qkv, heads)
    b, n = qkv.shape[:2]
    cos, sin = cos.double(), sin.double()

    def one(u, w):
        nh = u * torch.rsqrt(u.pow(2).mean(-1, keepdim=True) + eps)
        a = (ste(nh, bf(nh)) if rnd else nh) * w.double()
        pc, ps = a * cos, rotate_half(a) * sin
        return (pc + ps).reshape(b * heads, n, d), (pc.abs() + ps.abs()).reshape(b * heads, n, d)
    q, tq = one(t[0], qw)
    k, tk = one(t[1], kw)
    return q, k, tq, tk, t[2].reshape(b * heads, n, d)


TIE = 2.0 ** -19      # relative f32 error allowed on an operand of a flip-prone rounding site (rsqrt, the sum of squares, the product: under 16 roundings)


def qknorm_rope_bwd(dq, dk, dv, qkv, qw, kw, cos, sin, heads, eps=EPS):
    """dq, dk [B*H,N,Dp], dv [B*H,N,D] -> dict: dqkv value [B,N,3 H D] before its rounding (the dv third exact), its f32 terms, dqw / dkw [D] with their terms
    and the allowance for the rows whose bf16(q * rq) sits within TIE of a tie (there either neighbour is a correct rounding: one ulp times |e|)."""
    t, d = _heads(qkv, heads)
    b, n = qkv.shape[:2]
    cos, sin = cos.double(), sin.double()
    out = {}

    def one(u, g, w, name):
        g = g.double()[..., :d].reshape(b, heads, n, d)
        e = g * cos + rotate_half_t(g * sin)                             # e0 = g0 c0 + g1 s1, e1 = g1 c1 - g0 s0
        ea = (g * cos).abs() + rotate_half_t(g * sin).abs()
        r = torch.rsqrt(u.pow(2).mean(-1, keepdim=True) + eps)
        nh = u * r
        nb = bf(nh)
        out["d%sw" % name] = (e * nb).sum((0, 1, 2))
        out["d%sw_terms" % name] = (ea * nb.abs()).sum((0, 1, 2))
        out["d%sw_flip" % name] = (ea * (bf(nh * (1 + TIE)) - bf(nh * (1 - TIE))).abs()).sum((0, 1, 2))
        dn = e * w.double()
        mean = (dn * nh).mean(-1, keepdim=True)
        tm = ea * w.double().abs()
        return r * (dn - nh * mean), r * (tm + nh.abs() * (tm * nh.abs()).mean(-1, keepdim=True))
    gq, tq = one(t[0], dq, qw, "q")
    gk, tk = one(t[1], dk, kw, "k")
    gv = dv.double().reshape(b, heads, n, d)
    back = lambda a, c, e_: torch.stack([a, c, e_]).permute(1, 3, 0, 2, 4).reshape(b, n, 3 * heads * d)
    out["dqkv"] = back(gq, gk, gv)
    out["dqkv_terms"] = back(tq, tk, torch.zeros_like(gv))
    return out


def rmsnorm_modulate_bwd(dres, da, x, w, scale, eps=EPS):
    """Backward of a = bf16(n w m + shift), n = x rs, m = bf16(1 + scale) (straight through both roundings) -> dict of values and terms:
    dx = dres + rs (g - n mean(g n)), g = da w m;  dshift[b] = sum_n da;  dscale[b] = sum_n da n w;  dw = sum_rows da m n."""
    x, w, da, dres = x.double(), w.double(), da.double(), dres.double()
    m = bf(1 + scale.double()).unsqueeze(1)
    rs = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    n = x * rs
    g = da * w * m
    o = {"dx": dres + rs * (g - n * (g * n).mean(-1, keepdim=True))}
    o["dx_terms"] = dres.abs() + rs * (g.abs() + n.abs() * (g * n).abs().mean(-1, keepdim=True))
    o["dshift"], o["dshift_terms"] = da.sum(1), da.abs().sum(1)
    o["dscale"], o["dscale_terms"] = (da * n * w).sum(1), (da * n * w).abs().sum(1)
    o["dw"], o["dw_terms"] = (da * m * n).sum((0, 1)), (da * m * n).abs().sum((0, 1))
    return o


# ---- depths: f32 roundings on the longest path, from the loops of csrc/dit.hip ----------------------------------------------------------
def _sw(c):
    return (c + 255) // 256


def rms_fwd_depth(c):
    """rmsnorm_modulate{,8}_kernel: ss = one square, a 3-level tree in the lane, one add per sweep (SW), 6 butterfly levels; rs = rsqrt(ss / C + eps) carries half
    of that plus the division, the add and rsqrt (2); then v * rs * g * m + shift: 3 products and one sum."""
    return (10 + _sw(c)) / 2 + 4 + 4


def rms_bwd_dx_depth(c):
    """rowstat: ss and s2 run 4 sequential adds per sweep and 6 butterfly levels over products of 1 (ss) and 3 (s2) roundings: L = 4 SW + 7, L' = 4 SW + 9;
    rs carries L / 2 + 3.  m2 = s2 * rs / C: L' + 2 + rs.  dx = o + rs * (g - nh * m2): the g path 5 + rs, the m2 path rs (nh) + L' + 2 + rs (m2) + 4 + rs.
    Together L' + 7 + 3 (L / 2 + 3) <= 10 SW + 36; the single-kernel fallback has the same chains (4 SW in the lane, 6 butterfly levels)."""
    return 10 * _sw(c) + 36


def rms_bwd_bps(batch):
    return min(32, max(4, 1024 // batch))


def rms_bwd_red_depth(which, batch, seq, c, accumulate=False):
    """dshift / dscale / dw: the rows a thread walks (two-kernel route: ceil(N / bps) in the apply kernel; fallback above 4096 tokens: ceil(N / (4 bps)) per wave
    and 2 for the wave-pair combine), then bps partials in the final kernel, for dw the batch and the accumulate add; dscale and dw terms carry nh = v * rs
    (1 + L / 2 + 3, L = 4 SW + 7) and two products."""
    bps = rms_bwd_bps(batch)
    rows = -(-seq // bps) if seq <= 4096 else -(-seq // (4 * bps)) + 2
    d = rows + bps
    if which != "dshift":
        d += 6 + (4 * _sw(c) + 7) / 2
    if which == "dw":
        d += batch + (1 if accumulate else 0)
    return d


def gated_bwd_depth(seq):
    """gated_residual_bwd_kernel: a product, ceil(N / 8) adds per token lane, 8 in the LDS combine."""
    return -(-seq // 8) + 9


QK_FWD_DEPTH = 12     # sum of squares: 8 in the lane + 4 butterfly levels (16-lane form; the generic one 1 + 6) over squares -> rq: 13 / 2 + 3; q * rq, * w, * cos, the sum: 4


def qk_bwd_nblk(rows, d, dp):
    per = 16 if (d % 8 == 0 and dp % 8 == 0) else 4
    return min(2048, -(-rows // per)), per


def qk_bwd_dx_depth():
    """e: 3; rq: 10 (as forward), used three times (nq, the outer factor; eq * nq); the mean: a product, 8 in the lane, 4 (6) butterfly levels, the division: 14;
    dn, nq * m, the difference, the outer product: 4."""
    return 3 + 3 * 10 + 14 + 4


def qk_bwd_dw_depth(rows, d, dp):
    """the rows one lane walks (ceil(rows / (nblk * per))), the block's combine (16 sequential, or 2 levels), colsum2 (ceil(nblk / 16) sequential + 16), and per
    term e (3), rq (10) and the product."""
    nblk, per = qk_bwd_nblk(rows, d, dp)
    return -(-rows // (nblk * per)) + 16 + -(-nblk // 16) + 16 + 14


# ---- bars -----------------------------------------------------------------------------------------------------------------------------
def _report(what, err, bound, bad):
    flat = torch.where(bad.reshape(-1), (err / bound.clamp_min(1e-300)).reshape(-1).nan_to_num(float("inf")), torch.zeros((), dtype=err.dtype, device=err.device))
    i = int(flat.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape)) if err.dim() else ()
    return "%s: %d of %d elements out of bound; worst at %s: |error| %.6g against a bound of %.6g" % (
        what, int(bad.sum()), bad.numel(), idx, float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]))


def worst_ratio(y, ref, bound):
    return float(((y.double() - ref).abs() / bound.clamp_min(1e-300)).max())


def bf16_bound(ref, terms, depth, sites=None):
    """1.01 * 2^-8 * (|ref| + the terms of the flip-prone sites) + depth * 2^-24 * terms"""
    t = ref.abs() if sites is None else ref.abs() + sites
    return 1.01 * U8 * t + depth * U24 * terms


def check_bf16(y, ref, terms, depth, what, sites=None):
    """y (bf16) against the unrounded fp64 value `ref`, element by element: |y - ref| <= 1.01 * 2^-8 * sum_k |t_k| + depth * 2^-24 * terms, where t_k = |ref| for the
    result's own rounding and `sites` for the roundings inside the expression that the reference leaves unrounded."""
    assert y.dtype == BF and y.shape == ref.shape, (what, y.dtype, y.shape, ref.shape)
    err, bound = (y.double() - ref).abs(), bf16_bound(ref, terms, depth, sites)
    bad = ~(err <= bound)
    assert not bool(bad.any()), _report(what, err, bound, bad)


def check_f32(y, ref, terms, depth, what, extra=None):
    """y (f32) against fp64 `ref`: |y - ref| <= depth * 2^-24 * terms (+ `extra`, an allowance the caller derives), element by element."""
    assert y.dtype == torch.float32 and y.shape == ref.shape, (what, y.dtype, y.shape, ref.shape)
    err, bound = (y.double() - ref).abs(), depth * U24 * terms
    if extra is not None:
        bound = bound + extra
    bad = ~(err <= bound)
    assert not bool(bad.any()), _report(what, err, bound, bad)


def check_bf16_sites(y, s, rel, other, what):
    """y = bf16(bf16(s') * other) where s' is the kernel's f32 evaluation of `s`, within `rel` of it: the rounded factor is bf(s (1 - rel)) or bf(s (1 + rel))
    (one value except next to a tie), the product of two bf16 values is exact in f32, so y is within ONE half-ulp of a candidate product."""
    other = other.double()
    ok = torch.zeros_like(s, dtype=torch.bool)
    worst = torch.full_like(s, float("inf"))
    for c in (bf(s * (1 - rel)), bf(s * (1 + rel))):
        err, bound = (y.double() - c * other).abs(), 1.01 * U8 * (c * other).abs()
        ok |= err <= bound
        worst = torch.minimum(worst, err - bound)
    bad = ~ok
    assert not bool(bad.any()), _report(what, worst.clamp_min(0) + 1e-300, torch.full_like(s, 1e-300), bad)


def check_swiglu(y, x12, what="swiglu"):
    v, s = swiglu(x12, rnd=False)
    hid = s.shape[-1]
    x1 = x12[..., :hid]
    check_bf16(y, v, v.abs(), 0.0, what, sites=v.abs() * (1 + silu_err(x1) / U8))       # two roundings: 2^-7 |ref|, and the f32 error of silu
    check_bf16_sites(y, s, silu_err(x1), x12[..., hid:], what + " (rounded gate)")


def check_swiglu_bwd(dx12, dh, x12, what="swiglu_bwd"):
    v, terms, s = swiglu_bwd(dh, x12)
    hid = s.shape[-1]
    x1 = x12[..., :hid]
    su = dh.double() * s
    # dx1: one rounding; silu' carries the sigmoid's error (silu_err) and four products.  dx2: the gate's site and the result's rounding
    check_bf16(dx12[..., :hid], v[..., :hid], terms[..., :hid], 1.0, what + " dx1", sites=terms[..., :hid] * (silu_err(x1) + 4 * U24) / U8)
    check_bf16(dx12[..., hid:], su, su.abs(), 0.0, what + " dx2", sites=su.abs() * (1 + silu_err(x1) / U8))
    check_bf16_sites(dx12[..., hid:], s, silu_err(x1), dh, what + " dx2 (rounded gate)")


def check_qknorm_rope(q, k, v, qkv, qw, kw, cos, sin, heads, eps=EPS, what="qknorm_rope"):
    """q, k [B*H,N,Dp] (pad columns exactly zero), v [B*H,N,D]."""
    rq, rk, tq, tk, rv = qknorm_rope(qkv, qw, kw, cos, sin, heads, eps, rnd=False)
    d = rv.shape[-1]
    check_bf16(q[..., :d], rq, tq, QK_FWD_DEPTH, what + " q", sites=tq)
    check_bf16(k[..., :d], rk, tk, QK_FWD_DEPTH, what + " k", sites=tk)
    assert torch.equal(v.double(), rv), what + " v"
    if q.shape[-1] > d:
        assert not bool(q[..., d:].float().abs().max() > 0) and not bool(k[..., d:].float().abs().max() > 0), what + ": pad columns not zero"
        assert not bool(torch.signbit(q[..., d:].float()).any()), what + ": pad columns not +0"


def check_qknorm_rope_bwd(dqkv, dqw, dkw, dq, dk, dv, qkv, qw, kw, cos, sin, heads, eps=EPS, what="qknorm_rope_bwd"):
    o = qknorm_rope_bwd(dq, dk, dv, qkv, qw, kw, cos, sin, heads, eps)
    check_bf16(dqkv, o["dqkv"], o["dqkv_terms"], qk_bwd_dx_depth(), what + " dqkv")
    if dqw is not None:
        b, n = qkv.shape[:2]
        depth = qk_bwd_dw_depth(b * n * heads, dqw.numel(), dq.shape[-1])
        check_f32(dqw, o["dqw"], o["dqw_terms"], depth, what + " dq_weight", extra=o["dqw_flip"])
        check_f32(dkw, o["dkw"], o["dkw_terms"], depth, what + " dk_weight", extra=o["dkw_flip"])
    return o


def check_rmsnorm_modulate(y, x, w, scale, shift=None, eps=EPS, what="rmsnorm_modulate"):
    ref, terms = rmsnorm_modulate(x, w, scale, shift, eps)
    check_bf16(y, ref, terms, rms_fwd_depth(x.shape[-1]), what)


def check_rmsnorm_modulate_bwd(dx, dshift, dscale, dw, dres, da, x, w, scale, eps=EPS, dw0=None, what="rmsnorm_modulate_bwd"):
    """dshift None: the call had no shift chunk.  dw0: what dw held before an accumulating call."""
    b, n, c = x.shape
    o = rmsnorm_modulate_bwd(dres, da, x, w, scale, eps)
    check_f32(dx, o["dx"], o["dx_terms"], rms_bwd_dx_depth(c), what + " dx")
    if dshift is not None:
        check_f32(dshift, o["dshift"], o["dshift_terms"], rms_bwd_red_depth("dshift", b, n, c), what + " dshift")
    check_f32(dscale, o["dscale"], o["dscale_terms"], rms_bwd_red_depth("dscale", b, n, c), what + " dscale")
    acc = dw0 is not None
    check_f32(dw, o["dw"] + (dw0.double() if acc else 0), o["dw_terms"] + (dw0.double().abs() if acc else 0), rms_bwd_red_depth("dw", b, n, c, acc), what + " dw")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def hard_inputs(kind, t, **kw):
    """Edits `t` in place into the hard form of its kind and returns it; every intermediate of every kernel stays inside the normal f32 range.
      rows    [B,N,C] f32: row 0 all zero, row 1 scaled by 1e3, row 2 by 1e-3, row 3 = 1e-2 with a single 1e3 outlier (rows counted over B * N)
      scale   [B,C]: columns 0, 3, 6, ... = -1, 1, 4, ... = 2^-9 (bf16(1 + scale) == 1: tells a rounded 1 + scale from an unrounded one), 2, 5, ... left, and 0.5 at 5, 11, ...
      zero    [B,C]: the last sample all zero (shift = 0)
      gate    [B,C]: every fourth column zero
      silu    [rows, 2 hid]: x1 of the first columns cycles through -30, -8, -0.0, 0, 8, 30
      head    [B,N,3 H D] with heads=, which=: q of head `which` all zero"""
    if kind == "rows":
        f = t.view(-1, t.shape[-1])
        f[0] = 0
        if f.shape[0] > 1:
            f[1] *= 1e3
        if f.shape[0] > 2:
            f[2] *= 1e-3
        if f.shape[0] > 3:
            f[3] = 1e-2
            f[3, t.shape[-1] // 2] = 1e3
    elif kind == "scale":
        t[:, 0::3] = -1.0
        t[:, 1::3] = 2.0 ** -9
        t[:, 5::6] = 0.5
    elif kind == "zero":
        t[-1] = 0
    elif kind == "gate":
        t[:, 3::4] = 0
    elif kind == "silu":
        vals = torch.tensor([-30.0, -8.0, -0.0, 0.0, 8.0, 30.0], dtype=t.dtype)
        hid = t.shape[-1] // 2
        k = min(hid, 12)
        t[:, :k] = vals.repeat(2)[:k]
    elif kind == "head":
        heads, which = kw["heads"], kw["which"]
        b, n, c3 = t.shape
        t.view(b, n, 3, heads, c3 // 3 // heads)[:, :, 0, which] = 0
    else:
        raise ValueError(kind)
    return t


def rms_case(b, n, c, seed=0, hard=False, stride=None, shift_off=None, scale_off=None, gate_off=None, gstride=None):
    """The tensors of one RMSNorm / gated-residual case, on the CPU: x, dres [B,N,C] f32; r, da [B,N,C] bf16; w [C]; mod [B,stride], gmod [B,gstride] bf16 with the
    chunks at shift_off / scale_off / gate_off (defaults: the adaLN layout 0, C, 2C of a 6C row)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * b + 3 * n + c)
    stride = 6 * c if stride is None else stride
    gstride = stride if gstride is None else gstride
    shift_off = 0 if shift_off is None else shift_off
    scale_off = c if scale_off is None else scale_off
    gate_off = 2 * c if gate_off is None else gate_off
    x = torch.randn(b, n, c, generator=g) * 2
    r = torch.randn(b, n, c, generator=g)
    da = torch.randn(b, n, c, generator=g)
    dres = torch.randn(b, n, c, generator=g)
    w = 1 + 0.3 * torch.randn(c, generator=g)
    mod = 0.5 * torch.randn(b, stride, generator=g)
    gmod = 0.5 * torch.randn(b, gstride, generator=g)
    if hard:
        hard_inputs("rows", x)
        r.view(-1, c)[0] = 0                                    # the zero row stays zero through the gated prologue
        hard_inputs("scale", mod[:, scale_off:scale_off + c])
        hard_inputs("zero", mod[:, shift_off:shift_off + c])
        hard_inputs("gate", gmod[:, gate_off:gate_off + c])
    return dict(x=x, r=r.to(BF), da=da.to(BF), dres=dres, w=w, mod=mod.to(BF), gmod=gmod.to(BF), shift_off=shift_off, scale_off=scale_off, gate_off=gate_off, c=c)


def chunk(mod, off, c):
    return mod[:, off:off + c]


def swiglu_case(rows, hid, seed=0, hard=False):
    g = torch.Generator().manual_seed(2000 * seed + 5 * rows + hid)
    x12 = torch.randn(rows, 2 * hid, generator=g) * 2
    if hard:
        hard_inputs("silu", x12)
    return dict(x12=x12.to(BF), dh=torch.randn(rows, hid, generator=g).to(BF))


def qk_case(b, n, heads, d, dp=None, seed=0, hard=False):
    """dp None: the head dim rounded up to 32, as ops.qknorm_rope pads it.  cos and sin are INDEPENDENT random tables (c0 != c1, s0 != s1 within a feature pair)."""
    g = torch.Generator().manual_seed(3000 * seed + 11 * b + 5 * n + 3 * heads + d)
    dp = (d + 31) // 32 * 32 if dp is None else dp
    qkv = torch.randn(b, n, 3 * heads * d, generator=g) * 1.5
    if hard:
        hard_inputs("head", qkv, heads=heads, which=heads - 1)
    dq, dk = torch.zeros(b * heads, n, dp), torch.zeros(b * heads, n, dp)
    dq[..., :d] = torch.randn(b * heads, n, d, generator=g)
    dk[..., :d] = torch.randn(b * heads, n, d, generator=g)
    return dict(qkv=qkv.to(BF), qw=1 + 0.3 * torch.randn(d, generator=g), kw=1 + 0.3 * torch.randn(d, generator=g),
                cos=torch.rand(n, d, generator=g) * 2 - 1, sin=torch.rand(n, d, generator=g) * 2 - 1,
                dq=dq.to(BF), dk=dk.to(BF), dv=torch.randn(b * heads, n, d, generator=g).to(BF), heads=heads, d=d, dp=dp)


# ---- the cases of tests/test_gpu_dit_forms.py; the CPU emulation runs the ones marked small ------------------------------------------------
W4 = [4, 252, 260, 508, 516, 764, 772, 1020, 1028, 1276, 1284, 1532, 1540, 1788, 1796, 2044]       # four channels per lane: both edges of SW = 1 .. 6, 8
W8 = [8, 512, 520, 768, 1024, 1032, 1152, 1536, 1544, 2048]                                          # eight channels per lane: both edges of SW8 = 1 .. 4
RMS_FWD = [dict(b=3, n=5, c=c) for c in W4 + W8] + \
          [dict(b=7, n=1, c=c) for c in (260, 768)] + [dict(b=1, n=9, c=c) for c in (260, 768)] + \
          [dict(b=3, n=5, c=c, hard=True) for c in (260, 768, 1152)] + \
          [dict(b=3, n=5, c=1152, stride=6 * 1152 + 4, shift_off=4, scale_off=1152 + 4, gate_off=0, gstride=6 * 1152),               # the modulation's offsets 4 mod 8
           dict(b=3, n=5, c=1152, stride=6 * 1152, shift_off=0, scale_off=1152, gate_off=2 * 1152 + 4, gstride=6 * 1152 + 4)]        # the gate's
RMS_BWD = [dict(b=1, n=5, c=4), dict(b=1, n=33, c=252), dict(b=3, n=40, c=260), dict(b=40, n=64, c=1152), dict(b=300, n=3, c=516), dict(b=2, n=300, c=2044),
           dict(b=2, n=37, c=2048), dict(b=3, n=40, c=260, hard=True)]
RMS_BWD_FALLBACK = [dict(b=1, n=4097, c=c) for c in (8, 260, 516, 772, 1028, 1284, 1540, 2048)] + [dict(b=2, n=4100, c=8)]
GATED = [dict(b=b, n=n, c=c) for c in (8, 264, 1152, 2048) for n in (1, 7, 37) for b in (1, 5)]
SWIGLU = [dict(rows=r, hid=h) for h in (8, 40, 3072) for r in (1, 7, 300)]
QK_GENERIC = [dict(b=1, n=3, heads=1, d=2), dict(b=2, n=5, heads=3, d=6), dict(b=1, n=7, heads=5, d=36), dict(b=2, n=3, heads=3, d=70), dict(b=1, n=5, heads=3, d=126)]
QK_GENERIC_LOOP = dict(b=1, n=1367, heads=6, d=6)                     # 8,202 rows > 4 x 2048 blocks
QK16 = [dict(b=1, n=3, heads=3, d=8), dict(b=2, n=5, heads=3, d=72), dict(b=2, n=5, heads=3, d=72, dp=72), dict(b=1, n=7, heads=3, d=120), dict(b=1, n=5, heads=1, d=128)]
QK16_LOOP = dict(b=2, n=1025, heads=16, d=8)                          # 32,800 rows > 16 x 2048 blocks
QK_HARD = [dict(b=2, n=5, heads=3, d=6, hard=True), dict(b=2, n=5, heads=3, d=72, hard=True)]


def case_id(c):
    return "-".join("%s%s" % (k, v) for k, v in c.items())
