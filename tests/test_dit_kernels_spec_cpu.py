"""tests/dit_kernels_spec.py on the CPU: (1) its fp64 definitions against this project's stock modules in double and the CPU oracle, and its backward formulas
against autograd / gradcheck; (2) an f32 emulation of every kernel's arithmetic (from the comments of csrc/dit.hip) on the inputs of tests/test_gpu_dit_forms.py
passes every bar -- the bars can be met and the inputs are fair; (3) the same emulation with one seeded value-only defect fails the bar that guards it."""
import pytest
import torch
import torch.nn.functional as F

import dit_kernels_spec as S
from dit_kernels_spec import BF, EPS

D64 = torch.float64


# ---- (1) the spec is right ------------------------------------------------------------------------------------------------------------
def test_bf_is_the_bf16_rounding():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g), torch.tensor([0.0, -0.0, 1 + 2.0 ** -9, 1 + 3 * 2.0 ** -9, 1 - 2.0 ** -10])])
    assert torch.equal(S.bf(x.double()), x.to(BF).double())
    assert float(S.bf(torch.tensor(1 + 2.0 ** -9, dtype=D64))) == 1.0           # the tie goes to even: the hard scale


def test_rmsnorm_modulate_and_gate_against_the_stock_modules():
    from dmvae_amd.models.lightningdit import RMSNorm, modulate
    c = S.rms_case(3, 5, 260, hard=True)
    sh, sc, gt = (S.chunk(c["mod"], c[k], 260).double() for k in ("shift_off", "scale_off", "gate_off"))
    norm = RMSNorm(260).double()
    with torch.no_grad():
        norm.weight.copy_(c["w"].double())
        want = modulate(norm(c["x"].double()), sh, sc)
        want_ns = modulate(norm(c["x"].double()), None, sc)
    got, _ = S.rmsnorm_modulate(c["x"], c["w"], sc, sh, rnd=False)
    got_ns, _ = S.rmsnorm_modulate(c["x"], c["w"], sc, None, rnd=False)
    tol = dict(rtol=4e-6, atol=4e-6)                                                # the module normalises in f32 whatever it is given (rms_norm.py:52)
    assert torch.allclose(got, want, **tol) and torch.allclose(got_ns, want_ns, **tol)
    # the rounding site: the autocast graph's bf16 tensor 1 + scale
    m = (1 + S.chunk(c["mod"], c["scale_off"], 260)).double()                    # bf16 + 1 in bf16 arithmetic
    nrm = norm(c["x"].double()).detach()
    got_r, _ = S.rmsnorm_modulate(c["x"], c["w"], sc, sh)
    assert torch.allclose(got_r, nrm * m.unsqueeze(1) + sh.unsqueeze(1), **tol)
    # gated residual: the block's x + gate.unsqueeze(1) * y with the bf16 product
    y = c["r"]
    want = c["x"].double() + (S.chunk(c["gmod"], c["gate_off"], 260).unsqueeze(1) * y).double()
    assert torch.equal(S.gated_residual_f64(c["x"], S.chunk(c["gmod"], c["gate_off"], 260), y), want)
    assert torch.equal(S.gated_residual_exact(c["x"], S.chunk(c["gmod"], c["gate_off"], 260), y).double(), want.float().double())


@pytest.mark.parametrize("heads,d,side", [(3, 8, 3), (2, 36, 2)])
def test_qknorm_rope_against_the_stock_modules_and_the_oracle(heads, d, side):
    from dmvae_amd.models.lightningdit import RMSNorm, VisionRotaryEmbeddingFast
    from oracle import ref_cpu as R
    n = side * side
    c = S.qk_case(2, n, heads, d)
    rope = VisionRotaryEmbeddingFast(dim=d // 2, pt_seq_len=side).double()
    qn, kn = RMSNorm(d).double(), RMSNorm(d).double()
    with torch.no_grad():
        qn.weight.copy_(c["qw"].double()); kn.weight.copy_(c["kw"].double())
        q5 = c["qkv"].double().view(2, n, 3, heads, d).permute(2, 0, 3, 1, 4)
        wq, wk = rope(qn(q5[0])), rope(kn(q5[1]))
    q, k, _, _, v = S.qknorm_rope(c["qkv"], c["qw"], c["kw"], rope.freqs_cos, rope.freqs_sin, heads, rnd=False)
    assert torch.allclose(q, wq.reshape(2 * heads, n, d), rtol=4e-6, atol=4e-6) and torch.allclose(k, wk.reshape(2 * heads, n, d), rtol=4e-6, atol=4e-6)
    assert torch.equal(v, q5[2].reshape(2 * heads, n, d))
    # the oracle (f32, bf16 at the norm's cast) with independent tables
    oq = R.rope_2d(R.rms_norm(c["qkv"].view(2, n, 3, heads, d).permute(2, 0, 3, 1, 4)[0], c["qw"], q=R.bf16_round), c["cos"], c["sin"])
    q, _, tq, _, _ = S.qknorm_rope(c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], heads)
    assert ((q - oq.double().reshape(2 * heads, n, d)).abs() <= 2.0 ** -7 * tq + 1e-6).all()     # f32 oracle: a rare flipped rounding of the normalised value
    assert ((q - oq.double().reshape(2 * heads, n, d)).abs() <= 1e-5 * tq + 1e-6).float().mean() > 0.98


def test_swiglu_against_silu():
    c = S.swiglu_case(7, 40, hard=True)
    x = c["x12"].double()
    v, s = S.swiglu(c["x12"], rnd=False)
    assert torch.equal(v, F.silu(x[:, :40]) * x[:, 40:]) and torch.equal(s, F.silu(x[:, :40]))
    v, _ = S.swiglu(c["x12"])
    assert torch.equal(v, S.bf(F.silu(x[:, :40])) * x[:, 40:])


def test_forward_definitions_pass_gradcheck_without_the_rounding_sites():
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=D64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x, w, sc, sh: S.rmsnorm_modulate(x, w, sc, sh, rnd=False)[0], (r(2, 3, 8), r(8), r(2, 8), r(2, 8)))
    assert torch.autograd.gradcheck(lambda x, gt, y: S.gated_residual_f64(x, gt, y, rnd=False), (r(2, 3, 8), r(2, 8), r(2, 3, 8)))
    assert torch.autograd.gradcheck(lambda x: S.swiglu(x, rnd=False)[0], (r(3, 16),))
    cos, sin = torch.rand(3, 6, generator=g, dtype=D64), torch.rand(3, 6, generator=g, dtype=D64)
    assert torch.autograd.gradcheck(lambda x, qw, kw: torch.cat(S.qknorm_rope(x, qw, kw, cos, sin, 2, rnd=False)[:2]), (r(1, 3, 36), r(6), r(6)))


def test_backward_formulas_are_the_straight_through_gradients():
    # rmsnorm_modulate
    c = S.rms_case(3, 7, 12, hard=True)
    sh, sc = S.chunk(c["mod"], c["shift_off"], 12), S.chunk(c["mod"], c["scale_off"], 12)
    x, w = c["x"].double().requires_grad_(True), c["w"].double().requires_grad_(True)
    shd, scd = sh.double().requires_grad_(True), sc.double().requires_grad_(True)
    S.rmsnorm_modulate(x, w, scd, shd)[0].backward(c["da"].double())
    o = S.rmsnorm_modulate_bwd(c["dres"], c["da"], c["x"], c["w"], sc)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-11, atol=1e-11 * float(b.abs().max()))
    assert close(o["dx"], c["dres"].double() + x.grad) and close(o["dw"], w.grad) and close(o["dshift"], shd.grad) and close(o["dscale"], scd.grad)
    # gated residual
    gt = S.chunk(c["gmod"], c["gate_off"], 12)
    gd, yd = gt.double().requires_grad_(True), c["r"].double().requires_grad_(True)
    S.gated_residual_f64(c["x"], gd, yd).backward(c["dres"].double())
    dy, dgate, _ = S.gated_residual_bwd(c["dres"], gt, c["r"])
    assert close(dgate, gd.grad) and torch.equal(dy, yd.grad.to(BF))
    # swiglu
    s = S.swiglu_case(7, 40, hard=True)
    xd = s["x12"].double().requires_grad_(True)
    S.swiglu(xd)[0].backward(s["dh"].double())
    assert close(S.swiglu_bwd(s["dh"], s["x12"])[0], xd.grad)
    # qknorm_rope
    for q in (S.qk_case(2, 5, 3, 6, hard=True), S.qk_case(2, 5, 3, 72)):
        d = q["d"]
        xd, qw, kw = q["qkv"].double().requires_grad_(True), q["qw"].double().requires_grad_(True), q["kw"].double().requires_grad_(True)
        rq, rk, _, _, rv = S.qknorm_rope(xd, qw, kw, q["cos"], q["sin"], 3)
        ((rq * q["dq"][..., :d].double()).sum() + (rk * q["dk"][..., :d].double()).sum() + (rv * q["dv"].double()).sum()).backward()
        o = S.qknorm_rope_bwd(q["dq"], q["dk"], q["dv"], q["qkv"], q["qw"], q["kw"], q["cos"], q["sin"], 3)
        assert close(o["dqkv"], xd.grad) and close(o["dqw"], qw.grad) and close(o["dkw"], kw.grad)


# ---- (2), (3): the f32 emulation of the kernels' arithmetic, with seeded defects ------------------------------------------------------------
# defects: 1 `1 + scale` not rounded; 2 c0 for c1 in the second rotation component; 3 +s0 for -s0 in the transpose rotation; 4 mean over Dp; 5 the last row group
# left at its input; 6 silu not rounded; 7 dw without the last sample's partial; 8 the sample of a row taken as row / (rows_per_sample + 1)
def _sample(b, n, defect):
    return torch.arange(b * n) // (n + 1 if defect == 8 else n)


def emu_rms_fwd(c, gated, shift, defect=0):
    """-> (x after the gated prologue [B,N,C] f32, y bf16)"""
    x = c["x"].clone()
    b, n, w_ = x.shape
    s = _sample(b, n, defect)
    xf = x.view(-1, w_)
    if gated:
        xf = xf + (S.chunk(c["gmod"], c["gate_off"], w_)[s].float() * c["r"].view(-1, w_).float()).to(BF).float()
    rs = torch.rsqrt((xf * xf).sum(-1, keepdim=True) / w_ + EPS)
    m = 1 + S.chunk(c["mod"], c["scale_off"], w_)[s].float()
    if defect != 1:
        m = m.to(BF).float()
    sh = S.chunk(c["mod"], c["shift_off"], w_)[s].float() if shift else 0.0
    y = (xf * rs * c["w"] * m + sh).to(BF)
    if defect == 5:
        y[-4:] = c["x"].view(-1, w_)[-4:].to(BF)
        xf[-4:] = c["x"].view(-1, w_)[-4:]
    return xf.view(b, n, w_), y.view(b, n, w_)


def emu_rms_bwd(c, shift, defect=0, dw0=None):
    x, da, dres, w = c["x"], c["da"].float(), c["dres"], c["w"]
    b, n, w_ = x.shape
    s = _sample(b, n, defect)
    m = (1 + S.chunk(c["mod"], c["scale_off"], w_)[s].float()).to(BF).float().view(b, n, w_)
    rs = torch.rsqrt((x * x).sum(-1, keepdim=True) / w_ + EPS)
    nh = x * rs
    g = da * w * m
    m2 = (g * nh).sum(-1, keepdim=True) / w_
    dx = dres + rs * (g - nh * m2)
    wp = (da * m * nh).sum(1)
    dw = (wp[:-1] if defect == 7 else wp).sum(0) + (dw0 if dw0 is not None else 0)
    if defect == 5:
        dx.view(-1, w_)[-4:] = dres.view(-1, w_)[-4:]
    return dx, (da.sum(1) if shift else None), (da * nh * w).sum(1), dw


def _pairs(t):
    return t[..., 0::2], t[..., 1::2]


def _last_rows_mask(b, n, heads, count):
    """[B*H, N] mask of the last `count` kernel rows (row = token * H + head)"""
    row = (torch.arange(b).view(b, 1, 1) * n + torch.arange(n).view(1, 1, n)) * heads + torch.arange(heads).view(1, heads, 1)
    return (row >= b * n * heads - count).reshape(b * heads, n)


def emu_qk_fwd(c, defect=0):
    b, n, heads, d, dp = c["qkv"].shape[0], c["qkv"].shape[1], c["heads"], c["d"], c["dp"]
    t = c["qkv"].float().view(b, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    c0, c1 = _pairs(c["cos"])
    s0, s1 = _pairs(c["sin"])

    def one(u, w):
        r = torch.rsqrt((u * u).sum(-1, keepdim=True) / (dp if defect == 4 else d) + EPS)
        a0, a1 = _pairs((u * r).to(BF).float() * w)
        o = torch.stack([a0 * c0 - a1 * s0, a1 * (c0 if defect == 2 else c1) + a0 * s1], -1).reshape(b * heads, n, d)
        if defect == 5:
            mk = _last_rows_mask(b, n, heads, 16)
            o[mk] = u.reshape(b * heads, n, d)[mk]
        return F.pad(o, (0, dp - d)).to(BF)
    return one(t[0], c["qw"]), one(t[1], c["kw"]), t[2].reshape(b * heads, n, d).to(BF)


def emu_qk_bwd(c, defect=0):
    b, n, heads, d = c["qkv"].shape[0], c["qkv"].shape[1], c["heads"], c["d"]
    t = c["qkv"].float().view(b, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    c0, c1 = _pairs(c["cos"])
    s0, s1 = _pairs(c["sin"])

    def one(u, g, w):
        g0, g1 = _pairs(g.float()[..., :d].reshape(b, heads, n, d))
        e = torch.stack([g0 * c0 + g1 * s1, g1 * c1 + g0 * s0 if defect == 3 else g1 * c1 - g0 * s0], -1).reshape(b, heads, n, d)
        r = torch.rsqrt((u * u).sum(-1, keepdim=True) / d + EPS)
        nh = u * r
        gw = (e * nh.to(BF).float()).sum((0, 1, 2))
        dn = e * w
        return r * (dn - nh * ((dn * nh).sum(-1, keepdim=True) / d)), gw
    gq, dqw = one(t[0], c["dq"], c["qw"])
    gk, dkw = one(t[1], c["dk"], c["kw"])
    gv = c["dv"].float().reshape(b, heads, n, d)
    dqkv = torch.stack([gq, gk, gv]).permute(1, 3, 0, 2, 4).reshape(b, n, 3 * heads * d).to(BF)
    if defect == 5:
        # rows are (token, head): the last 16 of them keep the input
        flat = dqkv.view(b * n, 3, heads, d).permute(0, 2, 1, 3).reshape(b * n * heads, 3, d)
        src = c["qkv"].view(b * n, 3, heads, d).permute(0, 2, 1, 3).reshape(b * n * heads, 3, d)
        flat[-16:] = src[-16:]
        dqkv = flat.view(b * n, heads, 3, d).permute(0, 2, 1, 3).reshape(b, n, 3 * heads * d).contiguous()
    return dqkv, dqw, dkw


def emu_swiglu(c, defect=0):
    x = c["x12"].float()
    hid = x.shape[-1] // 2
    s = x[:, :hid] * torch.sigmoid(x[:, :hid])
    return ((s if defect == 6 else s.to(BF).float()) * x[:, hid:]).to(BF)


def emu_swiglu_bwd(c, defect=0):
    x, d = c["x12"].float(), c["dh"].float()
    hid = x.shape[-1] // 2
    x1, x2 = x[:, :hid], x[:, hid:]
    sg = torch.sigmoid(x1)
    s = x1 * sg
    return torch.cat([(d * x2 * (sg * (1 + x1 * (1 - sg)))).to(BF), (d * (s if defect == 6 else s.to(BF).float())).to(BF)], -1)


def _check_rms_fwd(c, gated, shift, defect=0):
    w_ = c["c"]
    xn, y = emu_rms_fwd(c, gated, shift, defect)
    x_ref = S.gated_residual_exact(c["x"], S.chunk(c["gmod"], c["gate_off"], w_), c["r"]) if gated else c["x"]
    assert torch.equal(xn, x_ref), "residual stream"
    S.check_rmsnorm_modulate(y, x_ref, c["w"], S.chunk(c["mod"], c["scale_off"], w_), S.chunk(c["mod"], c["shift_off"], w_) if shift else None)


def _check_rms_bwd(c, shift, defect=0, dw0=None):
    w_ = c["c"]
    dx, dsh, dsc, dw = emu_rms_bwd(c, shift, defect, dw0)
    S.check_rmsnorm_modulate_bwd(dx, dsh, dsc, dw, c["dres"], c["da"], c["x"], c["w"], S.chunk(c["mod"], c["scale_off"], w_), dw0=dw0)


def _check_qk_fwd(c, defect=0):
    q, k, v = emu_qk_fwd(c, defect)
    S.check_qknorm_rope(q, k, v, c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], c["heads"])


def _check_qk_bwd(c, defect=0):
    dqkv, dqw, dkw = emu_qk_bwd(c, defect)
    S.check_qknorm_rope_bwd(dqkv, dqw, dkw, c["dq"], c["dk"], c["dv"], c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], c["heads"])


@pytest.mark.parametrize("case", S.RMS_FWD, ids=S.case_id)
def test_emulation_meets_the_bars_rmsnorm_forward(case):
    c = S.rms_case(**case)
    for gated in (False, True):
        for shift in (True, False):
            _check_rms_fwd(c, gated, shift)
    if case.get("hard"):
        _, y = emu_rms_fwd(c, False, True)
        assert torch.equal(y[0, 0], S.chunk(c["mod"], c["shift_off"], c["c"])[0])          # the all-zero row gives the shift


@pytest.mark.parametrize("case", S.RMS_BWD + S.RMS_BWD_FALLBACK[:2] + S.RMS_BWD_FALLBACK[-1:], ids=S.case_id)
def test_emulation_meets_the_bars_rmsnorm_backward(case):
    c = S.rms_case(**case)
    _check_rms_bwd(c, True)
    _check_rms_bwd(c, False, dw0=torch.linspace(-3, 3, c["c"]))


@pytest.mark.parametrize("case", S.GATED, ids=S.case_id)
def test_emulation_meets_the_bars_gated_residual(case):
    c = S.rms_case(hard=True, **case)
    gt = S.chunk(c["gmod"], c["gate_off"], c["c"])
    s = _sample(case["b"], case["n"], 0)
    x = c["x"] + (gt[s].view(case["b"], case["n"], -1).float() * c["r"].float()).to(BF).float()
    assert torch.equal(x, S.gated_residual_exact(c["x"], gt, c["r"]))
    assert torch.equal(x[..., 3::4], c["x"][..., 3::4])                                  # gate = 0: bit-unchanged
    assert ((x.double() - S.gated_residual_f64(c["x"], gt, c["r"])).abs() <= S.U24 * x.double().abs()).all()
    dy, dgate, terms = S.gated_residual_bwd(c["dres"], gt, c["r"])
    S.check_f32((c["dres"] * c["r"].float()).sum(1), dgate, terms, S.gated_bwd_depth(case["n"]), "dgate")


@pytest.mark.parametrize("case", S.SWIGLU, ids=S.case_id)
def test_emulation_meets_the_bars_swiglu(case):
    c = S.swiglu_case(hard=True, **case)
    S.check_swiglu(emu_swiglu(c), c["x12"])
    S.check_swiglu_bwd(emu_swiglu_bwd(c), c["dh"], c["x12"])


@pytest.mark.parametrize("case", S.QK_GENERIC + S.QK16 + S.QK_HARD + [S.QK_GENERIC_LOOP, S.QK16_LOOP], ids=S.case_id)
def test_emulation_meets_the_bars_qknorm_rope(case):
    c = S.qk_case(**case)
    _check_qk_fwd(c)
    _check_qk_bwd(c)


HARD260 = dict(b=3, n=5, c=260, hard=True)


def _caught(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def test_bars_have_teeth():
    """Each seeded value-only defect of the emulation fails the helper that guards it; the same call without the defect passes (the tests above)."""
    c = S.rms_case(**HARD260)
    _check_rms_fwd(c, True, True)
    _caught(_check_rms_fwd, c, False, True, defect=1)           # 1: 1 + scale not rounded (scale = 2^-9 columns)
    _caught(_check_rms_fwd, c, True, False, defect=1)
    _caught(_check_rms_fwd, c, False, True, defect=5)           # 5: last 4 rows left at the input
    _caught(_check_rms_fwd, c, True, True, defect=5)
    _caught(_check_rms_fwd, c, False, True, defect=8)           # 8: row / (rows_per_sample + 1)
    _caught(_check_rms_fwd, c, True, False, defect=8)
    cb = S.rms_case(b=3, n=40, c=260, hard=True)
    _check_rms_bwd(cb, True)
    _caught(_check_rms_bwd, cb, True, defect=7)                 # 7: dw without one sample's partial
    _caught(_check_rms_bwd, cb, True, defect=8)
    _caught(_check_rms_bwd, cb, True, defect=5)
    for case in (dict(b=2, n=5, heads=3, d=6), dict(b=2, n=5, heads=3, d=72)):
        q = S.qk_case(**case)
        _caught(_check_qk_fwd, q, defect=2)                     # 2: c0 for c1
        _caught(_check_qk_bwd, q, defect=3)                     # 3: +s0 for -s0
        _caught(_check_qk_fwd, q, defect=4)                     # 4: mean over Dp (6 -> 32, 72 -> 96)
        _caught(_check_qk_fwd, q, defect=5)                     # 5: the last 16 rows
        _caught(_check_qk_bwd, q, defect=5)
    s = S.swiglu_case(7, 40, hard=True)                          # 6: random gates are far from a tie almost everywhere: the unrounded gate moves the product by up to
    _caught(S.check_swiglu, emu_swiglu(s, defect=6), s["x12"])  #    a half-ulp of the gate on top of the result's own, which one final rounding cannot explain
    _caught(S.check_swiglu_bwd, emu_swiglu_bwd(s, defect=6), s["dh"], s["x12"])
