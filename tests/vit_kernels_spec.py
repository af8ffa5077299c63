"""Not a test: the fp64 restatement of the ViT encoder's row kernels (csrc/vit.hip, csrc/vit_bwd.hip, common.h::dmvae_gelu_f), the element-wise bars their outputs
are held to, and the inputs the tests share (tests/test_vit_kernels_spec_cpu.py, tests/test_gpu_vit_kernels.py).  Nothing here needs a GPU or imports dmvae_amd;
every function runs on the device of its operands.

Definitions: plain torch in float64 from the header comments of the two files.
  layernorm          y = (x - mean) * rstd * gamma + beta, held BEFORE its bf16 rounding; the fused form first x' = fma(ls, r, x) (one f32 rounding)
  layernorm_bwd      dx_io += rstd * (g - mean(g) - x_hat * mean(g * x_hat)), g = dy * gamma;  dgamma = sum_rows dy * x_hat;  dbeta = sum_rows dy
  layerscale_bwd     dy = bf16(gamma * dt): one f32 product and one rounding, bit-exact in torch;  dgamma = sum_rows dt * y
  gelu, gelu'        x Phi(x) and Phi(x) + x phi(x) with Phi(x) = erfc(-x / sqrt 2) / 2: no cancellation in the negative tail
  softmax            exp(scale s - max) / sum

Bars: every element at its own magnitude, |got - ref| <= bound with
  bound = 1.01 * 2^-8 * (|ref| + E) + E        for a bf16 output: the half-ulp of the value the kernel rounds, which lies within E of ref
  bound = E                                    for an f32 output
  E     = depth * 2^-24 * sum |terms|  (+ the LayerNorm mean term, + the documented approximation error of dmvae_gelu_f, + 2^-126 where a result may flush)
`depth` is the number of f32 roundings on the longest path to the element, counted from the kernels' loops by the depth functions below.  No constant is fitted.

The LayerNorm mean term.  The f32 mean of a row is off by at most delta = mean_depth(C) * 2^-24 * mean|x| (lane sums, six butterfly levels, the product with the
rounded 1 / C).  x - mean is then off by delta in every channel of the row alike; scaled by rstd that is eps_m = delta * rstd on x_hat.  Since sum(x - mean) = 0
the variance moves by exactly delta^2, so rstd shrinks by at most eps_m^2 / 2 relative (1 / sqrt(1 + u) >= 1 - u / 2).  Hence
  y       eps_m |gamma| + eps_m^2 / 2 |x_hat gamma|
  dx      rstd eps_m (mean|g x_hat| + |x_hat| mean|g|) + 3/2 eps_m^2 T        (x_hat in m2 and in the product; rstd three times; T = the terms of dx)
  dgamma  sum_rows |dy| (eps_m + eps_m^2 / 2 |x_hat|)
For a row of large common offset (100 + 0.01 randn) the term is what decides; for zero variance (rstd = 1 / sqrt(eps)) it is the whole bound on y - beta.

Worst |error| / bound of the f32 CPU emulations of tests/test_vit_kernels_spec_cpu.py over every shared case (the only arbiter the bars have):
  layernorm y 0.986 (fused 0.986); layernorm_bwd dx 0.061, dgamma 0.136, dbeta 0.143; layerscale_bwd dgamma 0.267; scale_residual 0.990 x the one-rounding bar;
  gelu 0.965 (against its approximant 0.965); gelu_bwd 0.984; softmax 0.986.  The bf16 figures are the half-ulp at the bottom of a binade under the factor 1.01;
  no bar needed widening."""
import torch

BF = torch.bfloat16
F32 = torch.float32
D64 = torch.float64
U8 = 2.0 ** -8          # half an ulp of bf16 relative to the value, at most (8 significand bits)
U24 = 2.0 ** -24        # one f32 rounding, relative
TINY = 2.0 ** -126      # the smallest normal f32: a result or an intermediate below it may flush to zero
EPS = 1e-6
LN_WIDTHS = [256, 384, 512, 768, 1024, 1280, 1536]
LN_CLASSES = ["randn", "offset", "outlier", "const"]
LN_MAX_BLOCKS = 256     # csrc/vit_bwd.hip

FIG = {}                # worst |error| / bound per bar over everything checked in this process


def note(key, ratio):
    FIG[key] = max(FIG.get(key, 0.0), ratio)
    return ratio


def _report(what, err, bound, bad):
    flat = torch.where(bad.reshape(-1), (err / bound.clamp_min(1e-300)).reshape(-1).nan_to_num(float("inf")), torch.zeros((), dtype=err.dtype, device=err.device))
    i = int(flat.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape)) if err.dim() else ()
    return "%s: %d of %d elements out of bound; worst at %s: |error| %.6g against a bound of %.6g" % (
        what, int(bad.sum()), bad.numel(), idx, float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]))


def hold(got, ref, bound, what, key=None):
    """|got - ref| <= bound for every element (a NaN anywhere fails); returns the worst |error| / bound and notes it under `key`."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), _report(what, err, bound, bad)
    return note(key or what, float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0)


def bf16_bound(ref, e):
    return 1.01 * U8 * (ref.abs() + e) + e


# ---- depths: f32 roundings on the longest path, from the loops of csrc/vit.hip and csrc/vit_bwd.hip ----------------------------------------
def _sw(c):
    return c // 256


def _tail(c):
    return 1 if c % 256 else 0


def _lane_adds(c):
    """sequential additions of one lane's channels into ss / s1 / s2: four per sweep, two in the half sweep"""
    return 4 * _sw(c) + 2 * _tail(c)


def mean_depth(c):
    """s += (v0 + v1) + (v2 + v3) per sweep (2 + SWEEPS), the half sweep's own add, 6 butterfly levels, the product with 1 / C and that constant's own rounding"""
    return 2 + _sw(c) + _tail(c) + 6 + 2


def rstd_depth(c):
    """var: d = x - mean enters its square twice (2), the square (1), the lane's adds, 6 butterfly levels, 1 / C (2), + eps (1); rstd carries half of that and
    rsqrt (2)"""
    return (_lane_adds(c) + 12) / 2 + 2


def ln_fwd_depth(c):
    """(x - mean) * rstd * gamma + beta: the difference, two products, the sum, and rstd"""
    return rstd_depth(c) + 4


def ln_bwd_dx_depth(c):
    """x_hat = (x - mean) * rstd: 2 + R.  m2: g (1), x_hat, the product (1), S = the lane's adds + 6 + 2 (1 / C).  dx = o + rstd * (g - m1 - x_hat * m2): the
    longest path runs through x_hat * m2 (x_hat + m2 + 1), the subtraction, rstd and its product, the add: 10 + 3 R + S."""
    return 10 + 3 * rstd_depth(c) + _lane_adds(c) + 8


def ln_bwd_nblk(rows):
    return min(LN_MAX_BLOCKS, (rows + 3) // 4)


def ln_bwd_red_depth(which, rows, c, accumulate=False):
    """dgamma / dbeta: the rows one wave walks (ceil(rows / (4 nblk))), the block's four waves (2), colsum_parts (ceil(nblk / 4) serial + 2), the accumulate add;
    a dgamma term is dy * x_hat: the product and x_hat (2 + R)"""
    nblk = ln_bwd_nblk(rows)
    d = -(-rows // (4 * nblk)) + 2 + -(-nblk // 4) + 2 + (1 if accumulate else 0)
    return d + (3 + rstd_depth(c) if which == "dgamma" else 0)


def ls_geometry(rows, c):
    """layerscale_bwd: c / 8 lanes per row, rpb = 256 / (c / 8) rows per block (the remaining threads idle), nblk = ceil(rows / (8 rpb)) capped at 256"""
    rpb = 256 // (c // 8)
    return rpb, max(1, min(LN_MAX_BLOCKS, -(-rows // (8 * rpb))))


def ls_bwd_depth(rows, c, accumulate=False):
    """the product, the rows one thread walks, the block's rpb serial adds, colsum_parts, the accumulate add"""
    rpb, nblk = ls_geometry(rows, c)
    return 1 + -(-rows // (nblk * rpb)) + rpb + -(-nblk // 4) + 2 + (1 if accumulate else 0)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
def ln_stats(x, eps=EPS):
    """-> x_hat, rstd, eps_m (the mean term on x_hat), all fp64, the last two [rows, 1]"""
    x = x.double()
    d = x - x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps)
    return d * rstd, rstd, mean_depth(x.shape[-1]) * U24 * x.abs().mean(-1, keepdim=True) * rstd


def scale_residual(x, r, ls):
    """x + ls * r in fp64"""
    return x.double() + ls.double() * r.double()


def layernorm(x, gamma, beta, eps=EPS):
    """-> (y before its rounding, its f32 error E)"""
    xh, _, em = ln_stats(x, eps)
    t = xh * gamma.double()
    terms = t.abs() + beta.double().abs()
    return t + beta.double(), ln_fwd_depth(x.shape[-1]) * U24 * terms + em * gamma.double().abs() + 0.5 * em * em * t.abs()


def check_layernorm(y, x, gamma, beta, what, eps=EPS, key="layernorm y"):
    assert y.dtype == BF, (what, y.dtype)
    ref, e = layernorm(x, gamma, beta, eps)
    return hold(y, ref, bf16_bound(ref, e), what, key)


def check_scale_residual(x_new, x, r, ls, what, key="scale_residual"):
    """one fma: a single rounding of the exact value"""
    assert x_new.dtype == F32, (what, x_new.dtype)
    ref = scale_residual(x, r, ls)
    return hold(x_new, ref, 1.01 * U24 * ref.abs(), what, key)


def layernorm_bwd(dres, dy, x, gamma, eps=EPS):
    """-> dict: dx, dgamma, dbeta (fp64) and their f32 errors *_e for a call without accumulation"""
    c = x.shape[-1]
    rows = x.numel() // c
    xh, rstd, em = ln_stats(x, eps)
    dy, dres, gm = dy.double(), dres.double(), gamma.double()
    g = dy * gm
    m1, m2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    ma, m2a = g.abs().mean(-1, keepdim=True), (g * xh).abs().mean(-1, keepdim=True)
    o = {"dx": dres + rstd * (g - m1 - xh * m2)}
    t = dres.abs() + rstd * (g.abs() + ma + xh.abs() * m2a)
    o["dx_e"] = ln_bwd_dx_depth(c) * U24 * t + rstd * em * (m2a + xh.abs() * ma) + 1.5 * em * em * t
    lead = tuple(range(x.dim() - 1))
    o["dgamma"], o["dbeta"] = (dy * xh).sum(lead), dy.sum(lead)
    o["dgamma_terms"], o["dbeta_terms"] = (dy * xh).abs().sum(lead), dy.abs().sum(lead)
    o["dgamma_mean"] = (dy.abs() * (em + 0.5 * em * em * xh.abs())).sum(lead)
    o["rows"] = rows
    return o


def check_layernorm_bwd(dx, dg, db, dres, dy, x, gamma, what, eps=EPS, dg0=None, db0=None, ref=None):
    """dg / db None: the call asked for no parameter gradients.  dg0 / db0: what the outputs held before an accumulating call.  ref: a layernorm_bwd() result
    to reuse."""
    c = x.shape[-1]
    o = layernorm_bwd(dres, dy, x, gamma, eps) if ref is None else ref
    assert dx.dtype == F32, (what, dx.dtype)
    hold(dx, o["dx"], o["dx_e"], what + " dx", "layernorm_bwd dx")
    if dg is not None:
        acc = dg0 is not None
        z = torch.zeros_like(o["dgamma"])
        g0, b0 = (dg0.double(), db0.double()) if acc else (z, z)
        assert dg.dtype == F32 and db.dtype == F32, (what, dg.dtype, db.dtype)
        hold(dg, o["dgamma"] + g0, ln_bwd_red_depth("dgamma", o["rows"], c, acc) * U24 * (o["dgamma_terms"] + g0.abs()) + o["dgamma_mean"], what + " dgamma",
             "layernorm_bwd dgamma")
        hold(db, o["dbeta"] + b0, ln_bwd_red_depth("dbeta", o["rows"], c, acc) * U24 * (o["dbeta_terms"] + b0.abs()), what + " dbeta", "layernorm_bwd dbeta")
    return o


# ---- LayerScale backward -------------------------------------------------------------------------------------------------------------------
def layerscale_dy(dt, gamma):
    """bit-exact: one f32 product, one rounding"""
    return (gamma.float() * dt.float()).to(BF)


def check_layerscale_bwd(dy, dg, dt, y, gamma, what, dg0=None):
    c = y.shape[-1]
    rows = y.numel() // c
    assert dy.dtype == BF and torch.equal(dy, layerscale_dy(dt, gamma)), what + ": dy is not bf16(gamma * dt)"
    p = (dt.double() * y.double()).reshape(rows, c)
    ref, terms = p.sum(0), p.abs().sum(0)
    if dg0 is not None:
        ref, terms = ref + dg0.double(), terms + dg0.double().abs()
    assert dg.dtype == F32, (what, dg.dtype)
    return hold(dg, ref, ls_bwd_depth(rows, c, dg0 is not None) * U24 * terms, what + " dgamma", "layerscale_bwd dgamma")


# ---- GELU ----------------------------------------------------------------------------------------------------------------------------------
RSQRT2 = 0.7071067811865476
RSQRT2PI = 0.3989422804014327
AS_P, AS_A = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)     # Abramowitz & Stegun 7.1.26
AS_ERR = 1.5e-7                                                                               # its documented |error| on erf


def gelu(x):
    x = x.double()
    return x * 0.5 * torch.special.erfc(-x * RSQRT2)


def gelu_grad(x):
    x = x.double()
    return 0.5 * torch.special.erfc(-x * RSQRT2) + x * RSQRT2PI * torch.exp(-0.5 * x * x)


def gelu_approximant(x):
    """dmvae_gelu_f in fp64: 0.5 x E for x < 0, 0.5 x (2 - E) otherwise, E = (a1 t + ... + a5 t^5) exp(-z^2), t = 1 / (1 + p z), z = |x| / sqrt 2"""
    x = x.double()
    z = x.abs() * RSQRT2
    t = 1 / (1 + AS_P * z)
    p = torch.zeros_like(t)
    for a in reversed(AS_A):
        p = (p + a) * t
    e = p * torch.exp(-z * z)
    return 0.5 * x * torch.where(x < 0, e, 2 - e)


def gelu_f32_err(x, ref):
    """f32 work of dmvae_gelu_f: z (1), the fma (1), rcp (1), four fma (4), p * t (1), the product with exp (1), 2 - e (1), 0.5 x * . (1): 11.  exp(-z^2): z^2
    carries z twice and its own rounding, the exponent's conversion to base 2 one more, each worth z^2 * 2^-24 relative on the power: 4 z^2; exp itself 2.  For
    x >= 0 the power is at most 1 against the 2 it is taken from: its z^2-fold error stays under 4 * 0.37 of |x| / 2 (z^2 exp(-z^2) <= 1 / e)."""
    z2 = (0.5 * x.double() ** 2).clamp_max(128.0)                # past exp(-128) the power is zero in f32 and the result below TINY
    return torch.where(x < 0, (13 + 4 * z2) * U24 * ref.abs(), 15 * U24 * x.double().abs())


def check_gelu(y, x, what):
    """Two bars: against exact GELU with the approximant's documented error |x| / 2 * 1.5e-7, and against the approximant itself at the relative accuracy of its
    product chain -- the second one is what holds the negative tail, where 1 - erf would lose every bit to cancellation."""
    assert y.dtype == BF, (what, y.dtype)
    assert bool(torch.isfinite(y.float()).all()), what + ": not finite"
    ref = gelu(x)
    e = gelu_f32_err(x, ref) + 0.5 * x.double().abs() * AS_ERR + TINY
    a = hold(y, ref, bf16_bound(ref, e), what, "gelu")
    apx = gelu_approximant(x)
    e = gelu_f32_err(x, apx) + TINY
    return a, hold(y, apx, bf16_bound(apx, e), what + " (against its approximant)", "gelu approximant")


def check_gelu_bwd(dx, dy, x, what):
    """dy * (A + B), A = 0.5 (1 + erf(x / sqrt 2)) as the kernel takes it (argument 1, erff 4, the add 1, the half exact, and the sum below: terms 0.5 (1 + |erf|)),
    B = x phi(x) (-0.5 x x: 2 roundings and the base-2 conversion, each x^2 / 2 on the power: 1.5 x^2; exp 2; three products), the sum (1), the product with dy (1)."""
    assert dx.dtype == BF, (what, dx.dtype)
    assert bool(torch.isfinite(dx.float()).all()), what + ": not finite"
    xd, d = x.double(), dy.double().abs()
    a_terms = 0.5 * (1 + torch.special.erf(xd * RSQRT2).abs())
    b = (xd * RSQRT2PI * torch.exp(-0.5 * xd * xd)).abs()
    x2 = (xd * xd).clamp_max(256.0)                               # past exp(-128) B is zero in f32 and below TINY in fp64
    ref = dy.double() * gelu_grad(x)
    e = d * U24 * (6 * a_terms + (5 + 1.5 * x2) * b + 2 * (a_terms + b)) + TINY * (1 + d)
    return hold(dx, ref, bf16_bound(ref, e), what, "gelu_bwd")


# ---- softmax -------------------------------------------------------------------------------------------------------------------------------
def check_softmax(p, s, scale, what):
    """v = scale * s (1), d = v - max (1), the base-2 conversion (|d| on the power), exp (2): 4 + |d| per power, taken as 4 + 2 |d|; the sum: 8 in the lane, 6
    butterfly levels, over powers weighted by their share; the division and the product (2).  A power below TINY may flush."""
    assert p.dtype == BF and p.shape == s.shape, (what, p.dtype, p.shape)
    v = s.double() * scale
    d = v - v.max(-1, keepdim=True).values
    ref = torch.softmax(d, -1)
    own = 4 + 2 * d.abs().clamp_max(256.0)
    depth = own + (ref * own).sum(-1, keepdim=True) + 14 + 2
    a = hold(p, ref, bf16_bound(ref, depth * U24 * ref + TINY), what, "softmax")
    cols = s.shape[-1]
    rs = p.float().sum(-1)
    assert bool(((rs - 1).abs() <= cols * 2.0 ** -9).all()), what + ": a row's sum is off 1 by more than cols * 2^-9 (worst %.3g)" % float((rs - 1).abs().max())
    return a


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ln_rows(kind, rows, c, g):
    if kind == "randn":
        return torch.randn(rows, c, generator=g) * 2 + 0.3
    if kind == "offset":
        return 100 + 0.01 * torch.randn(rows, c, generator=g)
    if kind == "outlier":
        x = torch.randn(rows, c, generator=g)
        x[:, 3], x[:, c // 2], x[:, c - 1] = 400.0, -250.0, 600.0           # c - 1: the half sweep at 384, the last sweep elsewhere
        return x
    if kind == "const":
        return torch.full((rows, c), 3.0)
    raise ValueError(kind)


def ln_case(kind, rows, c):
    """x [rows, C] f32 of its class; x0 f32 with fma(ls, r, x0) ~ x (the stream in front of the fused form: its result keeps the class, up to a rounding);
    gamma with both signs, beta, ls [C] f32; r, dy bf16; dres f32 (what dx_io holds before the call); dg0, db0 the pre-fill of the accumulate form."""
    g = _gen(LN_CLASSES.index(kind), rows, c)
    x = ln_rows(kind, rows, c, g)
    gamma = 1 + 0.3 * torch.randn(c, generator=g)
    gamma[1::5] *= -1
    beta = 0.5 * torch.randn(c, generator=g)
    ls = 0.3 * torch.randn(c, generator=g)
    r = torch.randn(rows, c, generator=g).to(BF)
    x0 = (x.double() - ls.double() * r.double()).float()
    return dict(kind=kind, rows=rows, c=c, x=x, x0=x0, gamma=gamma, beta=beta, ls=ls, r=r, dy=torch.randn(rows, c, generator=g).to(BF),
                dres=torch.randn(rows, c, generator=g), dg0=torch.linspace(-3, 3, c), db0=torch.linspace(2, -2, c))


LN_FWD_ROWS = [1, 3, 4, 5, 1030]         # one block = four one-wave rows: 1, 3 and 5 leave idle waves in the last block
LN_FWD_HARD = (5, 1030)
LN_BWD_ROWS = [1, 5, 1024, 1027, 2500]   # 256 blocks = 1024 waves: at 1027 three waves take a second row, at 2500 the third round is ragged
LN_BWD_HARD = (5, 1027)


def ln_cases(rows_list, hard_rows):
    return [(k, r) for r in rows_list for k in (LN_CLASSES if r in hard_rows else LN_CLASSES[:1])]


LS_WIDTHS = [8, 256, 384, 512, 768, 1024, 1280, 1536, 2048]


def ls_rows(c):
    return [1, 7, 8 * ls_geometry(1, c)[0] + 1, 2100]


def ls_case(rows, c):
    g = _gen(77, rows, c)
    gamma = 0.5 * torch.randn(c, generator=g)
    return dict(rows=rows, c=c, dt=torch.randn(rows, c, generator=g) * 1.7, y=torch.randn(rows, c, generator=g).to(BF), gamma=gamma, dg0=torch.linspace(-3, 3, c))


def all_finite_bf16():
    """every finite bf16 value, subnormals and both zeros included: 65,280 of them, a multiple of 8"""
    bits = torch.arange(-32768, 32768, dtype=torch.int32)
    return bits[(bits & 0x7F80) != 0x7F80].to(torch.int16).view(BF)


def gelu_dys(n):
    g = _gen(91, n)
    return {"1": torch.ones(n).to(BF), "-0.75": torch.full((n,), -0.75).to(BF), "random": torch.randn(n, generator=g).to(BF)}


SOFTMAX_COLS = [1, 17, 63, 64, 65, 257, 511, 512]
SOFTMAX_ROWS = [1, 5, 1031]
SOFTMAX_SCALE = 0.125
SOFTMAX_KINDS = ["randn", "dominant", "equal", "floor"]


def softmax_case(kind, rows, cols):
    g = _gen(55, SOFTMAX_KINDS.index(kind), rows, cols)
    if kind == "randn":
        s = torch.randn(rows, cols, generator=g) * 4
    elif kind == "dominant":                       # one score at 3e4: scaled 3750, exp overflows without the max subtraction
        s = torch.randn(rows, cols, generator=g)
        s[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] = 3e4
    elif kind == "equal":                          # exactly uniform up to one rounding
        s = (torch.randn(rows, 1, generator=g) * 4).expand(rows, cols).clone()
    elif kind == "floor":                          # everything at -3e4 but one element at 0
        s = torch.full((rows, cols), -3e4)
        s[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] = 0.0
    else:
        raise ValueError(kind)
    return s.to(BF)


def to_dev(c, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
