"""LightningDiT block variants without a GPU: this project's restatement (tests/dit_variants_spec.py) and the mirror's stock route against the fixtures captured
from the reference's own model (tools/capture_dit_variants_golden.py), the kernel-level definitions against plain torch in fp64, their bars against f32
emulations of the kernels' arithmetic, and the predicates that route a variant model."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dit_kernels_spec as S
import dit_variants_spec as V
from conftest import load_golden, rel_err

TAGS = list(V.CFGS)


def _grads_match(named, g, x_grad):
    assert rel_err(x_grad, g.t("dx")) < 1e-4
    full = g.sub("g.")
    assert len(full) == 6
    for k, v in full.items():
        assert rel_err(named[k].grad, v) < 2e-4, k
    for n, prm in named.items():
        if prm.grad is None:
            assert n == "pos_embed", n
            continue
        gn = g["gn." + n][0]
        if gn > 1e-4:
            assert abs(prm.grad.double().norm().item() - gn) < 1e-3 * gn, n
    assert {k[3:] for k in g if k.startswith("gn.")} == {n for n, p_ in named.items() if p_.grad is not None}      # absent parameters: no entry either side


@pytest.mark.parametrize("tag", TAGS)
def test_variant_spec_and_stock_module_reproduce_the_reference_capture(tag):
    g = load_golden(tag)
    m = V.build(tag, g)
    x, t, y = g.t("x"), g.t("t"), torch.from_numpy(np.asarray(g["y"]))
    # the spec in f32, forward and (through autograd) backward
    p = {k: v.detach().clone() for k, v in m.state_dict().items()}
    names = [n for n, _ in m.named_parameters()]
    for n in names:
        p[n].requires_grad_(n != "pos_embed")
    xo = x.clone().requires_grad_(True)
    yo = V.lightningdit_forward(xo, t, y, p, V.CFGS[tag])
    assert rel_err(yo.detach(), g.t("out")) < 2e-5
    yo.backward(g.t("dy"))
    _grads_match({n: p[n] for n in names}, g, xo.grad)
    # the mirror's stock route on the regenerated weights: constructor and state-dict compatibility
    xr = x.clone().requires_grad_(True)
    out = m.forward_stock(xr, t, y)
    assert rel_err(out.detach(), g.t("out")) < 2e-5
    out.backward(g.t("dy"))
    _grads_match(dict(m.named_parameters()), g, xr.grad)


@pytest.mark.parametrize("tag", TAGS)
def test_variant_spec_with_bf16_sites_stays_near_the_capture_and_is_differentiable(tag):
    """q = bf16_round: a few 1e-3 .. 1e-2 from the f32 capture (the bf16 floor of a two-block model), never equal to the f32 run, gradients finite"""
    from oracle import ref_cpu as R
    g = load_golden(tag)
    m = V.build(tag, g)
    x, t, y = g.t("x"), g.t("t"), torch.from_numpy(np.asarray(g["y"]))
    p = {k: v.detach().clone() for k, v in m.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    yo = V.lightningdit_forward(xo, t, y, p, V.CFGS[tag], q=R.bf16_round)
    e = ((yo.detach().double() - g.t("out").double()).norm() / g.t("out").double().norm()).item()
    assert 1e-4 < e < 3e-2, e
    yo.backward(g.t("dy"))
    assert torch.isfinite(xo.grad).all() and ((xo.grad.double() - g.t("dx").double()).norm() / g.t("dx").double().norm()).item() < 6e-2


def test_predicates_route_variants_and_keep_the_default_guards():
    from dmvae_amd.models import lightningdit_fast as fast, lightningdit_parity
    from dmvae_amd.models.lightningdit import LightningDiT
    from dmvae_amd.train import _batchable
    for tag, kw in V.CFGS.items():
        m = LightningDiT(**kw).eval()
        assert fast.variant_supported(m), tag
        assert not fast.structurally_supported(m), tag                    # the parity-mode / DitStackFn / one-token guard is not widened
        assert not lightningdit_parity.structurally_supported(m), tag
        assert _batchable(m) and not _batchable(m.train())
    m = LightningDiT(**V.CFG_LAYERNORM_QK).eval()
    assert not fast.variant_supported(m) and not fast.structurally_supported(m) and not _batchable(m)
    why = fast.refused_reason(m)
    assert "use_qknorm=True" in why and "use_rmsnorm=False" in why and "LayerNorm" in why
    default = LightningDiT(**V._BASE, hidden_size=192, num_heads=3).eval()
    assert fast.structurally_supported(default) and not fast.variant_supported(default) and _batchable(default)
    # shape limits are the default route's: an MLP inner width that is no multiple of 8 stays out (hidden 128: int(2/3 * 512) = 341)
    assert not fast.variant_supported(LightningDiT(**V._BASE, hidden_size=128, num_heads=2, use_qknorm=False))
    assert not fast.variant_supported(LightningDiT(**dict(V._BASE, input_size=5), hidden_size=192, num_heads=3, use_rope=False))      # 25 tokens


def test_one_block_function_and_one_train_loop():
    """The variant copies are gone, not aliased: `DitBlockFn` and `forward_train` serve every configuration."""
    from dmvae_amd import functional
    from dmvae_amd.models import lightningdit_fast as fast
    assert hasattr(functional, "DitBlockFn") and not hasattr(functional, "DitBlockVarFn")
    assert hasattr(fast, "forward_train") and not hasattr(fast, "_forward_train_variant")


def test_frozen_bit_identity_models_sit_in_the_attention_regime_they_are_named_for():
    """The shapes and configurations of test_gpu_dit_variants.py's frozen / trainable cases, by the predicates alone: each shape's attention regime, and that the
    kernels take every model (the default through `structurally_supported`, the two variants through `variant_supported`).  With the constructor's mlp_ratio of 4
    the SwiGLU widths of hidden 128 and 64 (341, 170) are no multiples of 8 and both predicates refuse: hence `MLP_RATIO`."""
    from dmvae_amd import ops
    from dmvae_amd.models import lightningdit_fast as fast
    from dmvae_amd.models.lightningdit import LightningDiT
    want = {"resident": (True, True), "streaming": (True, False), "composed": (False, True)}      # (fused attention, within the resident kernels' tokens)
    assert set(V.FROZEN_SHAPES) == set(want)
    for name, (hidden, heads, side) in V.FROZEN_SHAPES.items():
        n, d = side * side, hidden // heads
        assert (ops.attention_heads_supported(n, d), n <= ops.ATTENTION_RESIDENT_MAX) == want[name], name
        for cname, sw in V.FROZEN_CONFIGS.items():
            m = LightningDiT(**V.frozen_case_cfg(name), **sw).eval()
            assert (fast.structurally_supported(m), fast.variant_supported(m)) == ((True, False) if cname == "default" else (False, True)), (name, cname)
            four = LightningDiT(**dict(V.frozen_case_cfg(name), mlp_ratio=4.0), **sw)
            assert sw.get("use_swiglu", True) == (not (fast.structurally_supported(four) or fast.variant_supported(four))), (name, cname)


def test_forward_on_the_cpu_still_raises_without_the_opt_in(monkeypatch):
    from dmvae_amd._lib import DmvaeHipError
    from dmvae_amd.models.lightningdit import LightningDiT
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    m = LightningDiT(**V.CFGS["dit_var_plain"]).eval()
    with pytest.raises(DmvaeHipError):
        m(torch.zeros(1, 8, 8, 8), torch.zeros(1), torch.zeros(1, dtype=torch.long))


def test_mod_offsets():
    from dmvae_amd.functional import dit_mod_offsets
    assert dit_mod_offsets(192, False) == (0, 192, 384, 576, 768, 960)
    assert dit_mod_offsets(192, True) == (-1, 0, 192, -1, 384, 576)          # scale_msa | gate_msa | scale_mlp | gate_mlp


# ---- kernel-level definitions against plain torch in fp64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [64, 132])
@pytest.mark.parametrize("hard", [False, True])
def test_layernorm_definition_is_torch_layer_norm_and_modulate(c, hard):
    k = V.ln_case(3, 5, c, hard=hard)
    x = k["x"].double().requires_grad_(True)
    sc, sh = S.chunk(k["mod"], k["scale_off"], c).double().requires_grad_(True), S.chunk(k["mod"], k["shift_off"], c).double().requires_grad_(True)
    ref = F.layer_norm(x, (c,), eps=1e-6) * (1 + sc).unsqueeze(1) + sh.unsqueeze(1)
    val, terms = V.layernorm_modulate(k["x"], sc.detach(), sh.detach(), rnd=False)
    assert torch.allclose(val, ref.detach(), rtol=1e-11, atol=1e-11) and bool((terms >= val.abs() * (1 - 1e-12)).all())
    val2, _ = V.layernorm_modulate(k["x"], sc.detach(), None, rnd=False)
    assert torch.allclose(val2, (F.layer_norm(x, (c,), eps=1e-6) * (1 + sc).unsqueeze(1)).detach(), rtol=1e-11, atol=1e-11)
    # the closed-form backward is autograd's, with bf16(1 + scale) as the multiplier value
    m = 1 + sc
    m = S.ste(m, S.bf(m))
    (F.layer_norm(x, (c,), eps=1e-6) * m.unsqueeze(1) + sh.unsqueeze(1)).backward(k["da"].double())
    o = V.layernorm_modulate_bwd(k["dres"], k["da"], k["x"], sc.detach())
    assert torch.allclose(o["dx"] - k["dres"].double(), x.grad, rtol=1e-9, atol=1e-9 * float(x.grad.abs().max()))
    assert torch.allclose(o["dscale"], sc.grad, rtol=1e-9, atol=1e-9) and torch.allclose(o["dshift"], sh.grad, rtol=1e-9, atol=1e-9)


def _rope_tables(side, d):
    from dmvae_amd.models.lightningdit import VisionRotaryEmbeddingFast
    rope = VisionRotaryEmbeddingFast(dim=d // 2, pt_seq_len=side).double()
    return rope, rope.freqs_cos, rope.freqs_sin


@pytest.mark.parametrize("norm,rope", [(False, True), (False, False), (True, False), (True, True)])
def test_head_split_definition_is_the_modules_and_its_backward_is_autograd(norm, rope):
    from dmvae_amd.models.lightningdit import RMSNorm
    heads, d, side = 2, 40, 4
    n = side * side
    k = S.qk_case(2, n, heads, d)
    rp, cos, sin = _rope_tables(side, d)
    qn = lambda u: u * torch.rsqrt(u.pow(2).mean(-1, keepdim=True) + RMSNorm(d).eps) * k["qw"].double()      # RMSNorm.forward's expression (the module itself computes in f32)
    qkv = k["qkv"].double()
    q5 = qkv.view(2, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    want = q5[0]
    if norm:
        want = qn(want)
    if rope:
        want = rp(want)
    kw = dict(qw=k["qw"] if norm else None, kw=k["kw"] if norm else None, cos=cos if rope else None, sin=sin if rope else None)
    q, _, tq, _, v = V.head_split(k["qkv"], heads, rnd=False, **kw)
    assert torch.allclose(q, want.reshape(2 * heads, n, d).detach(), rtol=1e-12, atol=1e-12) and bool((tq >= q.abs() * (1 - 1e-12)).all())
    assert torch.equal(v, q5[2].reshape(2 * heads, n, d))
    if norm and rope:                           # the default case: the existing definition
        q0 = S.qknorm_rope(k["qkv"], k["qw"], k["kw"], cos, sin, heads, rnd=False)[0]
        assert torch.equal(q, q0)
    # backward: the closed form against autograd over the definition with its straight-through rounding
    x = k["qkv"].double().requires_grad_(True)
    pw = {n_: (t.double().requires_grad_(True) if t is not None and n_ in ("qw", "kw") else t) for n_, t in kw.items()}
    qq, kk, _, _, vv = V.head_split(x, heads, rnd=True, **pw)
    ((qq * k["dq"][..., :d].double()).sum() + (kk * k["dk"][..., :d].double()).sum() + (vv * k["dv"].double()).sum()).backward()
    o = V.head_split_bwd(k["dq"], k["dk"], k["dv"], k["qkv"], heads, **kw)
    assert torch.allclose(o["dqkv"], x.grad, rtol=1e-10, atol=1e-10)
    if norm:
        assert torch.allclose(o["dqw"], pw["qw"].grad, rtol=1e-10, atol=1e-10) and torch.allclose(o["dkw"], pw["kw"].grad, rtol=1e-10, atol=1e-10)


def test_gelu_tanh_definition_is_torch_gelu_tanh():
    x = torch.cat([V.gelu_inputs(8 * 1024 + 3).double(), torch.linspace(-12, 12, 4001, dtype=torch.float64)]).requires_grad_(True)
    ref = F.gelu(x, approximate="tanh")
    val, _ = V.gelu_tanh(x.detach())
    assert torch.allclose(val, ref.detach(), rtol=1e-9, atol=1e-15)          # the sigmoid form has no cancellation: the tail differs in relative terms only
    ref.sum().backward()
    gr, terms, _, _ = V.gelu_tanh_grad(x.detach())
    assert torch.allclose(gr, x.grad, rtol=1e-9, atol=1e-12) and bool((terms >= gr.abs() * (1 - 1e-12)).all())


# ---- the bars against f32 emulations of the kernels' arithmetic (the only arbiter the bars have before a GPU run) ---------------------------
def _emulate_ln(x, scale, shift):
    """csrc/dit_variants.hip::ln_center + the output expression, in f32 torch (sums in torch's order, not the kernel's: the depth covers either)"""
    x = x.float()
    c = x.shape[-1]
    m0 = x.sum(-1, keepdim=True) / c
    d = x - m0
    d = d - d.sum(-1, keepdim=True) / c
    rs = torch.rsqrt((d * d).sum(-1, keepdim=True) / c + 1e-6)
    m = (1 + scale.float()).to(S.BF).float().unsqueeze(1)
    o = d * rs * m
    return (o if shift is None else o + shift.float().unsqueeze(1)).to(S.BF), (m0, d, rs)


@pytest.mark.parametrize("c", [64, 132, 1152, 2048])
@pytest.mark.parametrize("hard", [False, True])
def test_layernorm_bars_hold_an_f32_emulation_and_refuse_a_one_pass_variance(c, hard):
    k = V.ln_case(3, 5, c, hard=hard)
    sc, sh = S.chunk(k["mod"], k["scale_off"], c), S.chunk(k["mod"], k["shift_off"], c)
    y, (m0, d, rs) = _emulate_ln(k["x"], sc, sh)
    V.check_layernorm_modulate(y, k["x"], sc, sh)
    V.check_layernorm_modulate(_emulate_ln(k["x"], sc, None)[0], k["x"], sc, None)
    if hard:                                    # E[x^2] - mean^2 in f32: no digits left at x = 100 + 0.01 randn -- the bar must see it
        x = k["x"].float()
        var1 = ((x * x).mean(-1, keepdim=True) - x.mean(-1, keepdim=True) ** 2).clamp_min(0)
        bad = ((x - x.mean(-1, keepdim=True)) * torch.rsqrt(var1 + 1e-6) * (1 + sc.float()).to(S.BF).float().unsqueeze(1) + sh.float().unsqueeze(1)).to(S.BF)
        with pytest.raises(AssertionError):
            V.check_layernorm_modulate(bad, k["x"], sc, sh)
    # backward, emulated in f32 with the same deviation
    da, dres = k["da"].float(), k["dres"]
    m = (1 + sc.float()).to(S.BF).float().unsqueeze(1)
    xh = d * rs
    g = da * m
    dx = dres + rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    V.check_layernorm_modulate_bwd(dx, da.sum(1), (da * xh).sum(1), dres, k["da"], k["x"], sc)


def test_gelu_bars_hold_an_f32_emulation_and_refuse_the_erf_form():
    x = V.gelu_inputs(8 * 1024 + 3)
    xf = x.float()
    u = 0.7978845608028654 * (xf + 0.044715 * (xf * xf * xf))
    y = (xf * torch.sigmoid(2 * u)).to(S.BF)
    V.check_gelu_tanh(y, x)
    V.check_gelu_tanh(F.gelu(xf, approximate="tanh").to(S.BF)[xf > -3], x[xf > -3])      # torch's own f32 form, away from its cancelling tail
    with pytest.raises(AssertionError):
        V.check_gelu_tanh(F.gelu(xf).to(S.BF), x)                                        # the erf form is another function
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(S.BF)
    s = torch.sigmoid(2 * u)
    gr = s + xf * (2 * s * (1 - s)) * (0.7978845608028654 * (1 + 0.134145 * xf * xf))
    V.check_gelu_tanh_bwd((dy.float() * gr).to(S.BF), dy, x)


@pytest.mark.parametrize("norm,rope", [(False, True), (False, False), (True, False)])
def test_head_split_bars_hold_an_f32_emulation(norm, rope):
    heads, d, n = 2, 40, 5
    k = S.qk_case(2, n, heads, d)
    kw = dict(qw=k["qw"] if norm else None, kw=k["kw"] if norm else None, cos=k["cos"] if rope else None, sin=k["sin"] if rope else None)
    t = k["qkv"].float().view(2, n, 3, heads, d).permute(2, 0, 3, 1, 4)

    def one(u, w):
        if norm:
            u = (u * torch.rsqrt((u * u).mean(-1, keepdim=True) + 1e-6)).to(S.BF).float() * w
        if rope:
            u = u * k["cos"] + S.rotate_half(u) * k["sin"]
        return F.pad(u.reshape(2 * heads, n, d), (0, 64 - d)).to(S.BF)
    V.check_head_split(one(t[0], k["qw"]), one(t[1], k["kw"]), t[2].reshape(2 * heads, n, d).to(S.BF), k["qkv"], heads, **kw)
