"""tests/vit_kernels_spec.py on the CPU: (1) its fp64 definitions against torch's own layer_norm, gelu and softmax with autograd in float64; (2) an f32 emulation of
every kernel's arithmetic, in the kernel's order of operations (two-pass statistics, lane sums and the 64-lane butterfly, per-block partials and the fixed-order
combine), passes every bar on every shared case -- the bars can be met and the inputs are fair; (3) each deliberately wrong emulation fails the bar that guards it.
Run with -s to see the worst |error| / bound per bar (the figures recorded in the spec's docstring)."""
import pytest
import torch
import torch.nn.functional as F

import vit_kernels_spec as S
from vit_kernels_spec import BF, D64, EPS, F32


def _fig(*keys):
    for k in keys:
        if k in S.FIG:
            print("[fig] emulation, %s: worst |err| / bound %.3f (bar 1)" % (k, S.FIG[k]))


# ---- (1) the definitions against torch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.LN_CLASSES)
def test_layernorm_definitions_against_torch_autograd(kind):
    c = S.ln_case(kind, 5, 384)
    x, gm, bt = (c[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = F.layer_norm(x, (384,), gm, bt, EPS)
    y.backward(c["dy"].double())
    ref, _ = S.layernorm(c["x"], c["gamma"], c["beta"])
    close = lambda a, b: torch.allclose(a, b, rtol=1e-9, atol=1e-9 * float(b.abs().max()) + 1e-300)
    assert close(ref, y.detach())
    o = S.layernorm_bwd(c["dres"], c["dy"], c["x"], c["gamma"])
    assert close(o["dx"], c["dres"].double() + x.grad) and close(o["dgamma"], gm.grad) and close(o["dbeta"], bt.grad)
    if kind == "const":
        assert torch.equal(ref, c["beta"].double().expand_as(ref))                       # zero variance: y is beta


def test_layerscale_and_scale_residual_definitions_against_torch_autograd():
    c = S.ls_case(7, 384)
    x = torch.randn(7, 384, generator=torch.Generator().manual_seed(3))
    gm, y = c["gamma"].double().requires_grad_(True), c["y"].double().requires_grad_(True)
    out = x.double() + gm * y
    assert torch.equal(out.detach(), S.scale_residual(x, c["y"], c["gamma"]))
    out.backward(c["dt"].double())
    assert torch.equal(S.layerscale_dy(c["dt"], c["gamma"]), (c["gamma"] * c["dt"]).to(BF))
    assert ((S.layerscale_dy(c["dt"], c["gamma"]).double() - y.grad).abs() <= S.U8 * y.grad.abs()).all()
    assert torch.allclose((c["dt"].double() * c["y"].double()).sum(0), gm.grad, rtol=1e-12, atol=1e-12)


def test_gelu_definitions_against_torch_autograd():
    x = S.all_finite_bf16().double().requires_grad_(True)
    y = F.gelu(x)
    y.backward(torch.ones_like(y))
    pos = x.detach() > -5                     # torch takes the negative tail as 1 + erf: it agrees where that has bits left, and is bounded by 2^-53 |x| beyond
    assert torch.allclose(S.gelu(x.detach())[pos], y.detach()[pos], rtol=1e-9, atol=0)
    assert ((S.gelu(x.detach()) - y.detach()).abs() <= 2.0 ** -52 * x.detach().abs()).all()
    assert ((S.gelu_grad(x.detach()) - x.grad).abs() <= 2.0 ** -50).all()
    assert torch.allclose(S.gelu_grad(x.detach())[pos], x.grad[pos], rtol=1e-9, atol=1e-300)
    xs = torch.tensor([-30.0, -10.0, -6.0], dtype=D64)                                     # the tail against the asymptotic series phi(x) / |x| (1 - 1 / x^2 + 3 / x^4)
    tail = -S.RSQRT2PI * torch.exp(-0.5 * xs * xs) * (1 - 1 / xs ** 2 + 3 / xs ** 4)
    assert torch.allclose(S.gelu(xs), tail, rtol=15 / 6.0 ** 6, atol=0)
    # the approximant is within its documented error of the definition
    xa = S.all_finite_bf16().double()
    assert ((S.gelu_approximant(xa) - S.gelu(xa)).abs() <= 0.5 * xa.abs() * S.AS_ERR).all()


def test_softmax_definition_against_torch():
    s = S.softmax_case("randn", 5, 257)
    ref = torch.softmax(s.double() * S.SOFTMAX_SCALE, -1)
    S.check_softmax(ref.to(BF), s, S.SOFTMAX_SCALE, "torch softmax")


# ---- (2) the f32 emulations ----------------------------------------------------------------------------------------------------------------
def _wave_sum(v):
    """[..., 64] -> [..., 1]: the xor butterfly, every lane ends with the same sum"""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., :1]


def _lanes(x):
    """[rows, C] -> sweeps [rows, SWEEPS, 64, 4] and the half sweep [rows, 64, 2] or None"""
    rows, c = x.shape
    sw = c // 256
    return x[:, :sw * 256].reshape(rows, sw, 64, 4), (x[:, sw * 256:].reshape(rows, 64, 2) if c % 256 else None)


def _lane_seq(v, vt):
    """a lane's sequential sum over its channels: sweep by sweep, four per sweep, then the half sweep's two"""
    a = torch.zeros(v.shape[0], 64)
    for k in range(v.shape[1]):
        for e in range(4):
            a = a + v[:, k, :, e]
    if vt is not None:
        for e in range(2):
            a = a + vt[..., e]
    return a


def emu_stats(x, defect=None):
    """the kernels' two-pass statistics -> mean, rstd [rows, 1] f32"""
    rows, c = x.shape
    inv_c = torch.tensor(1.0 / c, dtype=F32)
    v, vt = _lanes(x)
    if defect == "no_half_sweep":
        vt = None
    s = torch.zeros(rows, 64)
    for k in range(v.shape[1]):
        s = s + ((v[:, k, :, 0] + v[:, k, :, 1]) + (v[:, k, :, 2] + v[:, k, :, 3]))
    if vt is not None:
        s = s + (vt[..., 0] + vt[..., 1])
    mean = _wave_sum(s) * inv_c
    if defect == "one_pass":
        ex2 = _wave_sum(_lane_seq(v * v, None if vt is None else vt * vt)) * inv_c
        return mean, torch.rsqrt(ex2 - mean * mean + EPS)
    d, dt = v - mean.view(rows, 1, 1, 1), (None if vt is None else vt - mean.view(rows, 1, 1))
    rstd = torch.rsqrt(_wave_sum(_lane_seq(d * d, None if dt is None else dt * dt)) * inv_c + EPS)
    if defect == "rstd_four_below":
        rstd = rstd[(torch.arange(rows) + 4).clamp_max(rows - 1)]
    return mean, rstd


def emu_fma(x, r, ls):
    """fmaf(ls, r, x): the product of an f32 and a bf16 value is exact in fp64, the sum rounds once there and once more to f32"""
    return (ls.double() * r.double() + x.double()).float()


def emu_layernorm(x, gamma, beta, defect=None):
    mean, rstd = emu_stats(x, defect)
    g = gamma
    if defect == "gamma_prev_sweep":            # lane 5's four channels of sweep 1 take sweep 0's gamma
        g = gamma.clone()
        g[256 + 20:256 + 24] = gamma[20:24]
    return ((x - mean) * rstd * g + beta).to(BF)


def _colsum_parts(part, out0, accumulate):
    """part [nblk, C] -> [C]: four interleaved groups, each serial over its blocks, combined as (0 + 1) + (2 + 3)"""
    nblk = part.shape[0]
    grp = []
    for k in range(4):
        a = torch.zeros(part.shape[1])
        for b in range(k, nblk, 4):
            a = a + part[b]
        grp.append(a)
    v = (grp[0] + grp[1]) + (grp[2] + grp[3])
    return (out0 if accumulate else torch.zeros_like(v)) + v


def emu_layernorm_bwd(dres, dy, x, gamma, dg0=None, db0=None, defect=None):
    rows, c = x.shape
    inv_c = torch.tensor(1.0 / c, dtype=F32)
    mean, rstd = emu_stats(x)
    xh = (x - mean) * rstd
    dyf = dy.float()
    g = dyf * gamma
    gv, gt = _lanes(g)
    pv, pt = _lanes(g * xh)
    m1 = _wave_sum(_lane_seq(gv, gt)) * inv_c
    m2 = _wave_sum(_lane_seq(pv, pt)) * inv_c
    dx = dres + rstd * (g - m1 - xh * m2)
    nblk = S.ln_bwd_nblk(rows)
    waves = 4 * nblk
    rounds = -(-rows // waves)
    pad = rounds * waves - rows
    ag = F.pad(dyf * xh, (0, 0, 0, pad)).view(rounds, waves, c)
    ab = F.pad(dyf, (0, 0, 0, pad)).view(rounds, waves, c)
    if defect == "last_round" and pad:
        rounds -= 1
    wg, wb = torch.zeros(waves, c), torch.zeros(waves, c)
    for k in range(rounds):
        wg, wb = wg + ag[k], wb + ab[k]
    wg, wb = wg.view(nblk, 4, c), wb.view(nblk, 4, c)
    part_g, part_b = (wg[:, 0] + wg[:, 1]) + (wg[:, 2] + wg[:, 3]), (wb[:, 0] + wb[:, 1]) + (wb[:, 2] + wb[:, 3])
    return dx, _colsum_parts(part_g, dg0, dg0 is not None), _colsum_parts(part_b, db0, db0 is not None)


def emu_layerscale_bwd(dt, y, gamma, dg0=None, defect=None):
    rows, c = y.shape
    rpb, nblk = S.ls_geometry(rows, c)
    per = nblk * rpb
    steps = -(-rows // per)
    p = F.pad(dt * y.float(), (0, 0, 0, steps * per - rows)).view(steps, nblk, rpb, c)
    acc = torch.zeros(nblk, rpb, c)
    for k in range(steps):
        acc = acc + p[k]
    part = torch.zeros(nblk, c)
    for r in range(rpb - 1 if defect == "last_block_row" else rpb):
        part = part + acc[:, r]
    return (gamma * dt).to(BF), _colsum_parts(part, dg0, dg0 is not None)


def emu_gelu(x, defect=None):
    x = x.float()
    if defect == "tanh":
        return (0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))).to(BF)
    z = x.abs() * 0.70710678118654752
    t = 1 / (S.AS_P * z + 1)
    p = torch.full_like(t, S.AS_A[4]) * t + S.AS_A[3]
    for a in (S.AS_A[2], S.AS_A[1], S.AS_A[0]):
        p = p * t + a
    e = p * t * torch.exp(-z * z)
    if defect == "one_minus_erf":
        erf = 1 - e
        return (0.5 * x * torch.where(x < 0, 1 - erf, 1 + erf)).to(BF)
    return (0.5 * x * torch.where(x < 0, e, 2 - e)).to(BF)


def emu_gelu_bwd(dy, x):
    x = x.float()
    return (dy.float() * (0.5 * (1 + torch.erf(x * 0.70710678118654752)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x))).to(BF)


def emu_softmax(s, scale, defect=None):
    rows, cols = s.shape
    v = F.pad(s.float() * scale, (0, 512 - cols), value=0.0 if defect == "zero_pad" else float("-inf")).view(rows, 8, 64)
    m = torch.zeros(rows, 1, 1) if defect == "no_max" else v.amax((1, 2), keepdim=True)
    e = torch.exp(v - m)
    a = torch.zeros(rows, 64)
    for k in range(8):
        a = a + e[:, k]
    inv = 1 / _wave_sum(a)
    return (e * inv.view(rows, 1, 1)).view(rows, 512)[:, :cols].to(BF)


def _ln_fwd(kind, rows, c, defect=None):
    k = S.ln_case(kind, rows, c)
    what = "%s rows %d width %d" % (kind, rows, c)
    S.check_layernorm(emu_layernorm(k["x"], k["gamma"], k["beta"], defect), k["x"], k["gamma"], k["beta"], what)
    xn = emu_fma(k["x0"], k["r"], k["ls"])
    S.check_scale_residual(xn, k["x0"], k["r"], k["ls"], what + " stream")
    S.check_layernorm(emu_layernorm(xn, k["gamma"], k["beta"], defect), xn, k["gamma"], k["beta"], what + " fused", key="layernorm y (fused)")


def _ln_bwd(kind, rows, c, defect=None):
    k = S.ln_case(kind, rows, c)
    what = "%s rows %d width %d" % (kind, rows, c)
    dx, dg, db = emu_layernorm_bwd(k["dres"], k["dy"], k["x"], k["gamma"], defect=defect)
    o = S.check_layernorm_bwd(dx, dg, db, k["dres"], k["dy"], k["x"], k["gamma"], what)
    dx, dg, db = emu_layernorm_bwd(k["dres"], k["dy"], k["x"], k["gamma"], k["dg0"], k["db0"], defect=defect)
    S.check_layernorm_bwd(dx, dg, db, k["dres"], k["dy"], k["x"], k["gamma"], what + " accumulate", dg0=k["dg0"], db0=k["db0"], ref=o)


def _ls(rows, c, defect=None):
    k = S.ls_case(rows, c)
    what = "rows %d width %d" % (rows, c)
    dy, dg = emu_layerscale_bwd(k["dt"], k["y"], k["gamma"], defect=defect)
    S.check_layerscale_bwd(dy, dg, k["dt"], k["y"], k["gamma"], what)
    dy, dg = emu_layerscale_bwd(k["dt"], k["y"], k["gamma"], k["dg0"], defect=defect)
    S.check_layerscale_bwd(dy, dg, k["dt"], k["y"], k["gamma"], what + " accumulate", dg0=k["dg0"])


@pytest.mark.parametrize("c", S.LN_WIDTHS)
def test_emulation_meets_the_bars_layernorm_forward(c):
    for kind, rows in S.ln_cases(S.LN_FWD_ROWS, S.LN_FWD_HARD):
        _ln_fwd(kind, rows, c)
    _fig("layernorm y", "layernorm y (fused)", "scale_residual")


@pytest.mark.parametrize("c", S.LN_WIDTHS)
def test_emulation_meets_the_bars_layernorm_backward(c):
    for kind, rows in S.ln_cases(S.LN_BWD_ROWS, S.LN_BWD_HARD):
        _ln_bwd(kind, rows, c)
    _fig("layernorm_bwd dx", "layernorm_bwd dgamma", "layernorm_bwd dbeta")


@pytest.mark.parametrize("c", S.LS_WIDTHS)
def test_emulation_meets_the_bars_layerscale_backward(c):
    for rows in S.ls_rows(c):
        _ls(rows, c)
    _fig("layerscale_bwd dgamma")


def test_emulation_meets_the_bars_gelu():
    x = S.all_finite_bf16()
    assert x.numel() == 65280
    S.check_gelu(emu_gelu(x), x, "gelu")
    for name, dy in S.gelu_dys(x.numel()).items():
        S.check_gelu_bwd(emu_gelu_bwd(dy, x), dy, x, "gelu_bwd dy=" + name)
    _fig("gelu", "gelu approximant", "gelu_bwd")


@pytest.mark.parametrize("cols", S.SOFTMAX_COLS)
def test_emulation_meets_the_bars_softmax(cols):
    for rows in S.SOFTMAX_ROWS:
        for kind in S.SOFTMAX_KINDS:
            s = S.softmax_case(kind, rows, cols)
            p = emu_softmax(s, S.SOFTMAX_SCALE)
            S.check_softmax(p, s, S.SOFTMAX_SCALE, "%s rows %d cols %d" % (kind, rows, cols))
            if kind == "equal":
                assert torch.equal(p, torch.tensor(1.0 / cols, dtype=F32).to(BF).expand(rows, cols))
    _fig("softmax")


# ---- (3) the negative controls -------------------------------------------------------------------------------------------------------------
def _caught(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def test_bars_have_teeth():
    """Each deliberately wrong emulation fails on a shared case; the same call without the defect passes (the tests above)."""
    _caught(_ln_fwd, "offset", 5, 256, defect="one_pass")                  # variance as E[x^2] - mean^2 in f32
    _caught(_ln_bwd_with_stats_defect, "offset", 5, 256, "one_pass")
    _caught(_ln_fwd, "randn", 5, 384, defect="no_half_sweep")              # columns >= 256 left out of the statistics
    _caught(_ln_fwd, "outlier", 1030, 384, defect="no_half_sweep")
    for c in (512, 1536):
        _caught(_ln_fwd, "randn", 5, c, defect="gamma_prev_sweep")         # one lane's four channels of sweep 1 with sweep 0's gamma
    _caught(_ln_fwd, "randn", 1030, 384, defect="rstd_four_below")         # a row's rstd from the row four below
    _caught(_ln_fwd, "randn", 5, 768, defect="rstd_four_below")
    for c in (384, 1280):
        _caught(_ln_bwd, "randn", 1027, c, defect="last_round")            # dgamma / dbeta without the three rows of the second round
        _caught(_ln_bwd, "randn", 2500, c, defect="last_round")            # ... without the ragged third round
    for rows in S.ls_rows(768)[1:]:
        _caught(_ls, rows, 768, defect="last_block_row")                   # row rpb - 1 of each block missing from dgamma
    s = S.softmax_case("dominant", 5, 65)
    _caught(S.check_softmax, emu_softmax(s, S.SOFTMAX_SCALE, "no_max"), s, S.SOFTMAX_SCALE, "no max")
    for cols in (17, 65, 257):
        s = S.softmax_case("randn", 5, cols)
        _caught(S.check_softmax, emu_softmax(s, S.SOFTMAX_SCALE, "zero_pad"), s, S.SOFTMAX_SCALE, "zero pad")
    x = S.all_finite_bf16()
    _caught(S.check_gelu, emu_gelu(x, "tanh"), x, "tanh form")
    _caught(S.check_gelu, emu_gelu(x, "one_minus_erf"), x, "1 - erf")


def _ln_bwd_with_stats_defect(kind, rows, c, defect):
    """the backward's x_hat from the defective statistics"""
    k = S.ln_case(kind, rows, c)
    mean, rstd = emu_stats(k["x"], defect)
    xh = (k["x"] - mean) * rstd
    g = k["dy"].float() * k["gamma"]
    dx = k["dres"] + rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    S.check_layernorm_bwd(dx, None, None, k["dres"], k["dy"], k["x"], k["gamma"], "one pass")
