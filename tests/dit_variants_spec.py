"""Not a test: this project's own CPU restatement of the LightningDiT block VARIANTS (the constructor's use_qknorm / use_swiglu / use_rope / use_rmsnorm /
wo_shift switches away from their defaults; diffusion/lightningdit/lightningdit.py:183-252, 258-274), the fp64 definitions of the kernels of
csrc/dit_variants.hip with the element-wise bars their outputs are held to, and the table of the `dit_var_*` fixtures (tools/capture_dit_variants_golden.py).
Shared by tests/test_dit_variants_cpu.py and tests/test_gpu_dit_variants.py; nothing here needs a GPU.

`lightningdit_forward(..., q=None)` is plain f32; with q = oracle.ref_cpu.bf16_round it rounds, straight through, where autocast(bf16) rounds in the reference's
graph.  Read off that graph for the variants:
  * nn.LayerNorm runs in f32 under autocast (its result is not rounded); `1 + scale` is a bf16 tensor; norm * (1 + scale) + shift is f32 and is rounded as the
    next Linear's input -- as for RMSNorm;
  * without QK-norm q and k are the qkv Linear's bf16 output; RoPE multiplies by f32 tables (f32 result) and scaled_dot_product_attention casts its operands to
    bf16: bf16(q cos + rotate_half(q) sin).  RMS-QK-norm without RoPE: bf16(bf16(q rq) * w);
  * nn.GELU(approximate="tanh") on the bf16 fc1 output: evaluated in f32, one rounding.

Kernel bars: the scheme of tests/dit_kernels_spec.py (whose helpers are used): a bf16 output against the UNROUNDED fp64 value, 1.01 * 2^-8 of the value plus
depth * 2^-24 * (sum of the magnitudes of the f32 terms), depth counted from the kernel's loops; f32 sums against fp64 with depth * 2^-24 * sum |terms|."""
import math

import torch
import torch.nn.functional as F

import dit_kernels_spec as S
from dit_kernels_spec import BF, EPS, U8, U24, bf, ste

_BASE = dict(input_size=8, patch_size=1, in_channels=8, depth=2, num_classes=10)
CFGS = {
    # the original DiT / SiT block: LayerNorm + GELU-MLP, no RoPE, no QK-norm, shift + scale + gate
    "dit_var_plain": dict(_BASE, hidden_size=192, num_heads=3, use_qknorm=False, use_swiglu=False, use_rope=False, use_rmsnorm=False, wo_shift=False),
    # the default without QK-norm (head dim 72)
    "dit_var_noqk": dict(_BASE, hidden_size=144, num_heads=2, use_qknorm=False),
    # the default without the shifts
    "dit_var_woshift": dict(_BASE, hidden_size=192, num_heads=3, wo_shift=True),
    "dit_var_mix_a": dict(_BASE, hidden_size=144, num_heads=2, use_rmsnorm=False, use_swiglu=True, use_rope=True, use_qknorm=False, wo_shift=True),
    "dit_var_mix_b": dict(_BASE, hidden_size=192, num_heads=3, use_rmsnorm=True, use_swiglu=False, use_rope=False, use_qknorm=True),
}
SEEDS = {"dit_var_plain": 81, "dit_var_noqk": 82, "dit_var_woshift": 83, "dit_var_mix_a": 84, "dit_var_mix_b": 85}
# the one combination that stays outside the kernels: an affine nn.LayerNorm(head_dim) on q and k
CFG_LAYERNORM_QK = dict(_BASE, hidden_size=192, num_heads=3, use_qknorm=True, use_rmsnorm=False)

# The frozen-against-trainable cases of test_gpu_dit_variants.py: (hidden, heads, grid side) per attention regime of `functional.DitBlockFn`, times three
# configurations.  Two things about these models follow from the predicates, not from a choice (test_dit_variants_cpu.py asserts both):
#  * the token count is a square that is a multiple of 32 (64, 256, 576, ...), so the smallest model above the resident kernels' 288 tokens has 24 x 24 = 576
#    -- a 320-token LightningDiT cannot be built;
#  * at the constructor's mlp_ratio = 4 the SwiGLU widths of hidden 128 and 64 are 341 and 170, no multiples of 8: mlp_ratio = 3 gives 256 and 128.
FROZEN_SHAPES = {"resident": (128, 2, 8), "streaming": (128, 2, 24), "composed": (64, 2, 8)}      # composed: head dim 32, outside the fused kernels
FROZEN_CONFIGS = {"default": {}, "noqk": dict(use_qknorm=False), "plain": dict(use_rmsnorm=False, use_qknorm=False, use_swiglu=False, wo_shift=True)}
MLP_RATIO = 3.0


def frozen_case_cfg(shape):
    hidden, heads, side = FROZEN_SHAPES[shape]
    return dict(input_size=side, patch_size=1, in_channels=16, hidden_size=hidden, depth=2, num_heads=heads, mlp_ratio=MLP_RATIO, num_classes=10)


def flags(kw):
    """the five switches of a configuration with the constructor's defaults filled in"""
    return dict(use_qknorm=kw.get("use_qknorm", True), use_swiglu=kw.get("use_swiglu", True), use_rope=kw.get("use_rope", True),
                use_rmsnorm=kw.get("use_rmsnorm", True), wo_shift=kw.get("wo_shift", False))


def full_gradient_names(kw):
    """the six parameters whose full gradients a fixture holds"""
    f = flags(kw)
    return ["blocks.0.adaLN_modulation.1.weight", "blocks.0.attn.q_norm.weight" if f["use_qknorm"] else "blocks.1.attn.qkv.bias",
            "blocks.0.mlp.w12.bias" if f["use_swiglu"] else "blocks.0.mlp.fc1.bias", "final_layer.linear.weight", "x_embedder.proj.weight", "t_embedder.mlp.0.weight"]


def build(tag, g, cfg=None):
    """this build's LightningDiT in the fixture's configuration with the fixture's deterministic weights (state-dict and constructor compatibility are asserted)"""
    from dmvae_amd.models.lightningdit import LightningDiT
    from oracle.detweights import det_fill_
    m = LightningDiT(**(CFGS[tag] if cfg is None else cfg)).eval()
    assert list(m.state_dict().keys()) == [str(k) for k in g["keys"]]
    for k, v in g.sub("fix.").items():
        assert torch.allclose(m.state_dict()[k], v, rtol=0, atol=2e-6), k
    det_fill_(m, int(g["seed"]), skip=("pos_embed",))
    return m


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def lightningdit_forward(x, t, y, p, cfg, q=None):
    """LightningDiT.forward in eval mode for any configuration of the five switches except LayerNorm-QK-norm.  p: state_dict; cfg: the constructor's keywords."""
    from oracle import ref_cpu as R
    _q, _qw = R._q, R._qw
    f = flags(cfg)
    num_heads, ps = cfg["num_heads"], cfg["patch_size"]
    b, c_in, hh, ww = x.shape
    hid = p["pos_embed"].shape[-1]
    hd = hid // num_heads
    lin = lambda v, name: _q(q, F.linear(_q(q, v), _qw(q, p[name + ".weight"]), p[name + ".bias"]))
    w = p["x_embedder.proj.weight"]
    pt = x.reshape(b, c_in, hh // ps, ps, ww // ps, ps).permute(0, 2, 4, 1, 3, 5).reshape(b, -1, c_in * ps ** 2)
    h = _q(q, F.linear(_q(q, pt), _qw(q, w.reshape(w.shape[0], -1)), p["x_embedder.proj.bias"])) + p["pos_embed"]
    half = 128
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    temb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    temb = lin(F.silu(lin(temb, "t_embedder.mlp.0")), "t_embedder.mlp.2")
    c = temb + p["y_embedder.embedding_table.weight"][y]

    def norm(v, name):      # f32 on the residual stream either way
        if f["use_rmsnorm"]:
            return R.rms_norm(v, p[name + ".weight"])
        return F.layer_norm(v, (hid,), eps=1e-6)

    def modulate(v, shift, scale):      # `1 + scale` is itself a bf16 tensor under autocast
        v = v * _q(q, 1 + scale.unsqueeze(1))
        return v if shift is None else v + shift.unsqueeze(1)

    def qk(v, name):
        if f["use_qknorm"]:
            v = R.rms_norm(v, p[name + ".weight"], q=q)
        if f["use_rope"]:
            v = R.rope_2d(v, p["feat_rope.freqs_cos"], p["feat_rope.freqs_sin"])
        return _q(q, v)
    nblk = 1 + max(int(k.split(".")[1]) for k in p if k.startswith("blocks."))
    for i in range(nblk):
        pre = f"blocks.{i}."
        mod = lin(F.silu(c), pre + "adaLN_modulation.1")
        if f["wo_shift"]:
            sc_a, g_a, sc_m, g_m = mod.chunk(4, dim=1)
            sh_a = sh_m = None
        else:
            sh_a, sc_a, g_a, sh_m, sc_m, g_m = mod.chunk(6, dim=1)
        qkv = lin(modulate(norm(h, pre + "norm1"), sh_a, sc_a), pre + "attn.qkv").reshape(b, -1, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
        att = torch.softmax((qk(qkv[0], pre + "attn.q_norm") @ qk(qkv[1], pre + "attn.k_norm").transpose(-2, -1)) * hd ** -0.5, dim=-1)
        o = _q(q, _q(q, att) @ qkv[2]).transpose(1, 2).reshape(b, -1, hid)
        h = h + _q(q, g_a.unsqueeze(1) * lin(o, pre + "attn.proj"))
        a = modulate(norm(h, pre + "norm2"), sh_m, sc_m)
        if f["use_swiglu"]:
            x1, x2 = lin(a, pre + "mlp.w12").chunk(2, dim=-1)
            mlp = lin(_q(q, _q(q, F.silu(x1)) * x2), pre + "mlp.w3")
        else:
            mlp = lin(_q(q, F.gelu(lin(a, pre + "mlp.fc1"), approximate="tanh")), pre + "mlp.fc2")
        h = h + _q(q, g_m.unsqueeze(1) * mlp)
    sh, sc = lin(F.silu(c), "final_layer.adaLN_modulation.1").chunk(2, dim=1)
    o = lin(modulate(norm(h, "final_layer.norm_final"), sh, sc), "final_layer.linear")
    gh = hh // ps
    c_out = o.shape[-1] // ps ** 2
    return o.reshape(b, gh, gh, ps, ps, c_out).permute(0, 5, 1, 3, 2, 4).reshape(b, c_out, hh, ww)


# ---- LayerNorm + modulate ----------------------------------------------------------------------------------------------------------------
def _sw(c):
    return (c + 255) // 256


def ln_sum_depth(c):
    """a row sum in ln_center: a 3-level tree in the lane, one add per sweep, 6 butterfly levels, the division"""
    return _sw(c) + 10


def _ln_parts(x, eps):
    x = x.double()
    c = x.shape[-1]
    d = x - x.mean(-1, keepdim=True)
    rs = torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps)
    # f32 error of the kernel's deviation, as a magnitude: the first mean is off by up to e0 = L 2^-24 mean|x|; the deviation from it is re-centred by a mean taken
    # over values of size |d| + e0 (error L 2^-24 of their mean magnitude), so d carries (L + 2) 2^-24 (|d| + mean|d| + e0) -- `dt` is that magnitude; rs carries the
    # relative error of the variance built from it, hence the factor (1 + e0 rs)
    e0 = ln_sum_depth(c) * U24 * x.abs().mean(-1, keepdim=True)
    dt = (d.abs() + d.abs().mean(-1, keepdim=True) + e0) * (1 + e0 * rs)
    return d, rs, dt


def layernorm_modulate(x, scale, shift=None, eps=EPS, rnd=True):
    """x [B,N,C], scale / shift [B,C] -> (value [B,N,C] before its bf16 rounding, terms)."""
    d, rs, dt = _ln_parts(x, eps)
    m = 1 + scale.double()
    if rnd:
        m = ste(m, bf(m))
    m = m.unsqueeze(1)
    t, terms = d * rs * m, dt * rs * m.abs()
    if shift is None:
        return t, terms
    sh = shift.double().unsqueeze(1)
    return t + sh, terms + sh.abs()


def ln_fwd_depth(c):
    """d: L + 2 (the mean, the subtraction, twice over: carried by `dt`); rs: the variance sum (a square, L) over deviations of 2 (L + 2) relative error, halved,
    plus the division, the add and rsqrt; then d * rs * m + shift: 2 products and a sum."""
    L = ln_sum_depth(c)
    return (L + 2) + ((L + 1) / 2 + (L + 2) + 3) + 3


def check_layernorm_modulate(y, x, scale, shift=None, eps=EPS, what="layernorm_modulate"):
    ref, terms = layernorm_modulate(x, scale, shift, eps)
    S.check_bf16(y, ref, terms, ln_fwd_depth(x.shape[-1]), what)


def layernorm_modulate_bwd(dres, da, x, scale, eps=EPS):
    """Backward of a = bf16(xh m + shift), xh = (x - mean) rs, m = bf16(1 + scale) (straight through both roundings) -> dict of values and terms:
    dx = dres + rs (g - mean(g) - xh mean(g xh)), g = da m;  dshift[b] = sum_n da;  dscale[b] = sum_n da xh."""
    da, dres = da.double(), dres.double()
    d, rs, dt = _ln_parts(x, eps)
    m = bf(1 + scale.double()).unsqueeze(1)
    xh, xt = d * rs, dt * rs
    g = da * m
    o = {"dx": dres + rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))}
    o["dx_terms"] = dres.abs() + rs * (g.abs() + g.abs().mean(-1, keepdim=True) + xt * (g.abs() * xt).mean(-1, keepdim=True))
    o["dshift"], o["dshift_terms"] = da.sum(1), da.abs().sum(1)
    o["dscale"], o["dscale_terms"] = (da * xh).sum(1), (da.abs() * xt).sum(1)
    return o


def ln_bwd_bps(batch):
    return min(32, max(4, 1024 // batch))


def ln_bwd_dx_depth(c):
    """xh: (L + 2) + rs (as the forward: (L + 1) / 2 + L + 5) + a product = H; mean(g): a product, 4 SW adds in the lane, 6 butterfly levels, the division;
    mean(g xh): the same over terms that carry H + 1; dx = o + rs (g m - m1 - xh m2): rs, the two means and xh once more, three sums and a product."""
    L = ln_sum_depth(c)
    H = (L + 2) + ((L + 1) / 2 + L + 5) + 1
    red = 4 * _sw(c) + 8
    return 2 * H + 2 * red + 8


def ln_bwd_red_depth(which, batch, seq, c):
    """dshift / dscale: the ceil(N / bps) rows a thread of the apply kernel walks, then the bps partials; dscale's terms carry xh (H) and a product."""
    bps = ln_bwd_bps(batch)
    d = -(-seq // bps) + bps
    if which == "dscale":
        L = ln_sum_depth(c)
        d += (L + 2) + ((L + 1) / 2 + L + 5) + 2
    return d


def check_layernorm_modulate_bwd(dx, dshift, dscale, dres, da, x, scale, eps=EPS, what="layernorm_modulate_bwd"):
    """dshift None: the call had no shift chunk."""
    b, n, c = x.shape
    o = layernorm_modulate_bwd(dres, da, x, scale, eps)
    S.check_f32(dx, o["dx"], o["dx_terms"], ln_bwd_dx_depth(c), what + " dx")
    if dshift is not None:
        S.check_f32(dshift, o["dshift"], o["dshift_terms"], ln_bwd_red_depth("dshift", b, n, c), what + " dshift")
    S.check_f32(dscale, o["dscale"], o["dscale_terms"], ln_bwd_red_depth("dscale", b, n, c), what + " dscale")
    return o


def ln_case(b, n, c, seed=0, hard=False, stride=None, shift_off=None, scale_off=None, gate_off=None):
    """One LayerNorm / gated-residual case on the CPU: x, dres [B,N,C] f32; r, da bf16; mod [B,stride] bf16 with the chunks at the given offsets (defaults: 0, C, 2C
    of a 6C row).  hard: every row a large common offset with a small spread, x = 100 + 0.01 randn -- E[x^2] - mean^2 in f32 has no digits left there."""
    g = torch.Generator().manual_seed(4000 * seed + 7 * b + 3 * n + c)
    stride = 6 * c if stride is None else stride
    shift_off = 0 if shift_off is None else shift_off
    scale_off = c if scale_off is None else scale_off
    gate_off = 2 * c if gate_off is None else gate_off
    x = torch.randn(b, n, c, generator=g) * 2
    if hard:
        x = 100 + 0.01 * torch.randn(b, n, c, generator=g)
    r = torch.randn(b, n, c, generator=g) * (0.01 if hard else 1.0)
    da = torch.randn(b, n, c, generator=g)
    dres = torch.randn(b, n, c, generator=g)
    mod = 0.5 * torch.randn(b, stride, generator=g)
    return dict(x=x, r=r.to(BF), da=da.to(BF), dres=dres, mod=mod.to(BF), shift_off=shift_off, scale_off=scale_off, gate_off=gate_off, c=c)


# ---- head split --------------------------------------------------------------------------------------------------------------------------
def head_split(qkv, heads, qw=None, kw=None, cos=None, sin=None, eps=EPS, rnd=True):
    """qkv [B,N,3 H D] -> (q, k values [B*H,N,D] before their rounding, their terms, v exact).  qw / kw: per-head RMSNorm, the normalised value rounded to bf16 before
    the weight multiplies; cos / sin [N,D]: t cos + rotate_half(t) sin."""
    t, d = S._heads(qkv, heads)
    b, n = qkv.shape[:2]

    def one(u, w):
        a = u
        if w is not None:
            nh = u * torch.rsqrt(u.pow(2).mean(-1, keepdim=True) + eps)
            a = (ste(nh, bf(nh)) if rnd else nh) * w.double()
        if cos is not None:
            pc, ps = a * cos.double(), S.rotate_half(a) * sin.double()
            return (pc + ps).reshape(b * heads, n, d), (pc.abs() + ps.abs()).reshape(b * heads, n, d)
        return a.reshape(b * heads, n, d), a.abs().reshape(b * heads, n, d)
    q, tq = one(t[0], qw)
    k, tk = one(t[1], kw)
    return q, k, tq, tk, t[2].reshape(b * heads, n, d)


def check_head_split(q, k, v, qkv, heads, qw=None, kw=None, cos=None, sin=None, eps=EPS, what="head_split"):
    """q, k [B*H,N,Dp] (pad columns exactly +0), v [B*H,N,D]."""
    rq, rk, tq, tk, rv = head_split(qkv, heads, qw, kw, cos, sin, eps, rnd=False)
    d = rv.shape[-1]
    assert q.dtype == BF and k.dtype == BF
    if qw is None and cos is None:              # a relayout: bit for bit
        assert torch.equal(q[..., :d].double(), rq) and torch.equal(k[..., :d].double(), rk), what + ": relayout not exact"
    elif qw is None:                            # two products and a sum on exact operands
        S.check_bf16(q[..., :d], rq, tq, 3, what + " q")
        S.check_bf16(k[..., :d], rk, tk, 3, what + " k")
    else:                                       # the rounding of the normalised value sits inside the expression (dit_kernels_spec.check_qknorm_rope)
        S.check_bf16(q[..., :d], rq, tq, S.QK_FWD_DEPTH, what + " q", sites=tq)
        S.check_bf16(k[..., :d], rk, tk, S.QK_FWD_DEPTH, what + " k", sites=tk)
    assert torch.equal(v.double(), rv), what + " v"
    if q.shape[-1] > d:
        assert not bool(q[..., d:].float().abs().max() > 0) and not bool(k[..., d:].float().abs().max() > 0), what + ": pad columns not zero"
        assert not bool(torch.signbit(q[..., d:].float()).any()) and not bool(torch.signbit(k[..., d:].float()).any()), what + ": pad columns not +0"


def head_split_bwd(dq, dk, dv, qkv, heads, qw=None, kw=None, cos=None, sin=None, eps=EPS):
    """dq, dk [B*H,N,Dp], dv [B*H,N,D] -> dict: dqkv value [B,N,3 H D] before its rounding (the dv third exact) and its f32 terms; with a norm dqw / dkw [D], their
    terms and the tie allowance of dit_kernels_spec.qknorm_rope_bwd.  The closed form of autograd over `head_split` (tests/test_dit_variants_cpu.py holds them equal)."""
    t, d = S._heads(qkv, heads)
    b, n = qkv.shape[:2]
    out = {}

    def one(u, g, w, name):
        g = g.double()[..., :d].reshape(b, heads, n, d)
        if cos is not None:
            e = g * cos.double() + S.rotate_half_t(g * sin.double())
            ea = (g * cos.double()).abs() + S.rotate_half_t(g * sin.double()).abs()
        else:
            e, ea = g, g.abs()
        if w is None:
            return e, ea
        r = torch.rsqrt(u.pow(2).mean(-1, keepdim=True) + eps)
        nh = u * r
        nb = bf(nh)
        out["d%sw" % name] = (e * nb).sum((0, 1, 2))
        out["d%sw_terms" % name] = (ea * nb.abs()).sum((0, 1, 2))
        out["d%sw_flip" % name] = (ea * (bf(nh * (1 + S.TIE)) - bf(nh * (1 - S.TIE))).abs()).sum((0, 1, 2))
        dn = e * w.double()
        tm = ea * w.double().abs()
        return r * (dn - nh * (dn * nh).mean(-1, keepdim=True)), r * (tm + nh.abs() * (tm * nh.abs()).mean(-1, keepdim=True))
    gq, tq = one(t[0], dq, qw, "q")
    gk, tk = one(t[1], dk, kw, "k")
    gv = dv.double().reshape(b, heads, n, d)
    back = lambda a, c, e_: torch.stack([a, c, e_]).permute(1, 3, 0, 2, 4).reshape(b, n, 3 * heads * d)
    out["dqkv"] = back(gq, gk, gv)
    out["dqkv_terms"] = back(tq, tk, torch.zeros_like(gv))
    return out


def head_split_bwd_dw_depth(rows):
    """the rows one wave walks (ceil(rows / (4 nblk)), nblk = min(2048, ceil(rows / 4))), the block's 4-wave combine (2), the second stage (ceil(nblk / 4) per chain
    + 2), and per term e (3), rq (10) and the product -- the generic kernel of csrc/dit_variants.hip."""
    nblk = min(2048, -(-rows // 4))
    return -(-rows // (4 * nblk)) + 2 + -(-nblk // 4) + 2 + 14


def check_head_split_bwd(dqkv, dqw, dkw, dq, dk, dv, qkv, heads, qw=None, kw=None, cos=None, sin=None, eps=EPS, what="head_split_bwd"):
    o = head_split_bwd(dq, dk, dv, qkv, heads, qw, kw, cos, sin, eps)
    assert dqkv.dtype == BF
    if qw is None and cos is None:
        assert torch.equal(dqkv.double(), o["dqkv"]), what + ": relayout not exact"
    else:
        S.check_bf16(dqkv, o["dqkv"], o["dqkv_terms"], 3 if qw is None else S.qk_bwd_dx_depth(), what + " dqkv")
    if qw is None:
        assert dqw is None and dkw is None
    else:
        b, n = qkv.shape[:2]
        depth = head_split_bwd_dw_depth(b * n * heads)
        S.check_f32(dqw, o["dqw"], o["dqw_terms"], depth, what + " dq_weight", extra=o["dqw_flip"])
        S.check_f32(dkw, o["dkw"], o["dkw_terms"], depth, what + " dk_weight", extra=o["dkw_flip"])
    return o


# ---- tanh-GELU ---------------------------------------------------------------------------------------------------------------------------
K0, K1 = math.sqrt(2.0 / math.pi), 0.044715
TINY = 2.0 ** -126      # the smallest normal f32: a sigmoid below it is a subnormal or flushed to zero -- an absolute error of up to TINY on s and on s (1 - s)


def gelu_tanh(x):
    """0.5 x (1 + tanh(u)), u = sqrt(2/pi) (x + 0.044715 x^3), in fp64 as x * sigmoid(2u) (the same function; no cancellation in the negative tail)."""
    x = x.double()
    u = K0 * (x + K1 * x ** 3)
    return x * torch.sigmoid(2 * u), u


def gelu_tanh_grad(x):
    """-> (d/dx, the magnitude of its two terms, u, the factors an absolute error of s and s (1 - s) is multiplied by)"""
    x = x.double()
    u = K0 * (x + K1 * x ** 3)
    s = torch.sigmoid(2 * u)
    t2 = x * 2 * s * (1 - s) * K0 * (1 + 3 * K1 * x * x)
    return s + t2, s + t2.abs(), u, 1 + (2 * x * K0 * (1 + 3 * K1 * x * x)).abs()


def gelu_err(u, extra=0.0):
    """Relative f32 error of the kernel's x * sigmoid(2u): u from five roundings (its error enters the exponent: 5 |2u| 2^-24 on the power), the fast exponential
    (1.5 |2u| + 8) 2^-24 as dit_kernels_spec.silu_err takes it, the add, the reciprocal and two products."""
    return (13.0 * u.abs() + 12.0 + extra) * U24


def check_gelu_tanh(y, x, what="gelu_tanh"):
    """finite inputs"""
    ref, u = gelu_tanh(x)
    assert y.dtype == BF and y.shape == x.shape
    err, bound = (y.double() - ref).abs(), (1.01 * U8 + gelu_err(u)) * ref.abs() + (x.double().abs() + 1) * TINY
    bad = ~(err <= bound)
    assert not bool(bad.any()), S._report(what, err, bound, bad)


def check_gelu_tanh_bwd(dx, dy, x, what="gelu_tanh_bwd"):
    gr, terms, u, amp = gelu_tanh_grad(x)
    ref = dy.double() * gr
    assert dx.dtype == BF and dx.shape == x.shape
    err, bound = (dx.double() - ref).abs(), 1.01 * U8 * ref.abs() + gelu_err(u, 8.0) * (dy.double().abs() * terms) + (dy.double().abs() * amp + 1) * TINY
    bad = ~(err <= bound)
    assert not bool(bad.any()), S._report(what, err, bound, bad)


def gelu_inputs(n, seed=0):
    """n bf16 values over [-12, 12] with +-0 among them"""
    g = torch.Generator().manual_seed(5000 + seed + n)
    x = (torch.rand(n, generator=g) * 24 - 12)
    x[::5] = torch.randn(x[::5].shape, generator=g)      # the interesting range densely
    if n >= 2:
        x[0], x[1] = 0.0, -0.0
    return x.to(BF)


GELU_SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.3895313892515355e38, -3.3895313892515355e38, 1e15, -1e15, 12.0, -12.0]
