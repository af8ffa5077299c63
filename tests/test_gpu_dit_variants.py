"""LightningDiT block variants on the HIP kernels (-m gpu): the kernels of csrc/dit_variants.hip against tests/dit_variants_spec.py, and `LightningDiT` in the
five captured configurations of its constructor's switches -- inference and training under autocast(bf16) -- against the reference's f32 capture
(tools/capture_dit_variants_golden.py), the bf16-site restatement and the stock modules.  Tolerances of the model-level tests are tests/test_gpu_dit.py's for the
same quantities; the kernel bars are derived in the spec file.  No test here opts in to the stock route."""
import functools

import numpy as np
import pytest
import torch

import dit_kernels_spec as S
import dit_variants_spec as V
from conftest import load_golden
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
Q = R.bf16_round
TAGS = list(V.CFGS)


def _rl2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _dev(k):
    return {n: (v.to(DEV) if torch.is_tensor(v) else v) for n, v in k.items()}


# ---- 1. kernels against the spec --------------------------------------------------------------------------------------------------------
LN_WIDTHS = [64, 132, 1152, 2048]        # less than a wave's 256 channels, four channels per lane only (132 % 8 != 0), five sweeps, the cap
LN_ROWS = [(3, 1), (3, 5), (3, 64)]      # rows that are no multiple of the four a workgroup takes


def _ln_layouts(c):
    """(stride, shift_off, scale_off, gate_off): the first chunks of a 6C row, the MLP chunks of a 6C row, and the two halves of a 4C (`wo_shift`) row with the shift
    taken from a neighbouring chunk so that the with-shift form is exercised at that stride too"""
    return [(6 * c, 0, c, 2 * c), (6 * c, 3 * c, 4 * c, 5 * c), (4 * c, c, 0, c), (4 * c, 3 * c, 2 * c, 3 * c)]


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("b,n", LN_ROWS)
@pytest.mark.parametrize("c", LN_WIDTHS)
def test_layernorm_modulate_forward_three_launch_forms(c, b, n, hard):
    from dmvae_amd import ops
    for stride, sh, sc, go in _ln_layouts(c):
        k = V.ln_case(b, n, c, seed=stride // c, hard=hard, stride=stride, shift_off=sh, scale_off=sc, gate_off=go)
        d = _dev(k)
        scale, shift = S.chunk(k["mod"], sc, c), S.chunk(k["mod"], sh, c)
        y = ops.layernorm_modulate(d["x"], d["mod"], sh, sc)
        V.check_layernorm_modulate(y.cpu(), k["x"], scale, shift, what=f"layernorm_modulate c{c} stride{stride}")
        y0 = ops.layernorm_modulate(d["x"], d["mod"], -1, sc)
        V.check_layernorm_modulate(y0.cpu(), k["x"], scale, None, what=f"layernorm_modulate (no shift) c{c} stride{stride}")
        assert torch.equal(y, ops.layernorm_modulate(d["x"], d["mod"], sh, sc))
        # fused with the preceding gated residual == the two kernels back to back, bit for bit; in place and out of place
        x1, none = ops.gated_residual_out(d["x"], d["r"], d["mod"], go)
        assert none is None
        assert torch.equal(x1, S.gated_residual_exact(d["x"], S.chunk(d["mod"], go, c), d["r"]))
        for s_off in (sh, -1):
            y1 = ops.layernorm_modulate(x1, d["mod"], s_off, sc)
            x2 = d["x"].clone()
            y2 = ops.gated_residual_layernorm_modulate_(x2, d["r"], d["mod"], go, d["mod"], s_off, sc)
            assert torch.equal(x2, x1) and torch.equal(y2, y1)
            xin = d["x"].clone()
            x3, y3 = ops.gated_residual_layernorm_out(xin, d["r"], d["mod"], go, d["mod"], s_off, sc)
            assert torch.equal(xin, d["x"]) and torch.equal(x3, x1) and torch.equal(y3, y1)
        V.check_layernorm_modulate(y1.cpu(), x1.cpu(), scale, None, what=f"gated residual + layernorm c{c} stride{stride}")


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("b,n", LN_ROWS)
@pytest.mark.parametrize("c", LN_WIDTHS)
def test_layernorm_modulate_backward(c, b, n, hard):
    from dmvae_amd import ops
    for stride, sh, sc, go in _ln_layouts(c)[1:3]:
        k = V.ln_case(b, n, c, seed=7 + stride // c, hard=hard, stride=stride, shift_off=sh, scale_off=sc, gate_off=go)
        d = _dev(k)
        scale = S.chunk(k["mod"], sc, c)
        for s_off in (sh, -1):
            dmod = torch.full((b, stride), 7.0, device=DEV)
            dx = d["dres"].clone()
            ops.layernorm_modulate_bwd_(dx, d["da"], d["x"], d["mod"], dmod, s_off, sc)
            dm = dmod.cpu()
            V.check_layernorm_modulate_bwd(dx.cpu(), S.chunk(dm, sh, c) if s_off >= 0 else None, S.chunk(dm, sc, c), k["dres"], k["da"], k["x"], scale,
                                           what=f"layernorm_modulate_bwd c{c} stride{stride} shift{s_off}")
            own = torch.zeros(stride, dtype=torch.bool)
            own[sc:sc + c] = True
            if s_off >= 0:
                own[sh:sh + c] = True
            assert bool((dm[:, ~own] == 7.0).all()), "layernorm_modulate_bwd wrote outside its chunks"
            dmod2 = torch.full((b, stride), 7.0, device=DEV)
            dx2 = d["dres"].clone()
            ops.layernorm_modulate_bwd_(dx2, d["da"], d["x"], d["mod"], dmod2, s_off, sc)
            assert torch.equal(dx2, dx) and torch.equal(dmod2, dmod)              # identical run to run


@pytest.mark.parametrize("b,n", LN_ROWS)
@pytest.mark.parametrize("c", LN_WIDTHS)
def test_rmsnorm_modulate_without_shift_forward_and_backward(c, b, n):
    """The existing RMSNorm kernels at shift_off < 0 inside a 4C (`wo_shift`) row: scale_msa at 0 and scale_mlp at 2C, nothing written to another chunk."""
    from dmvae_amd import ops
    for sc in (0, 2 * c):
        k = S.rms_case(b, n, c, seed=11, stride=4 * c, shift_off=0, scale_off=sc, gate_off=c)
        d = _dev(k)
        scale = S.chunk(k["mod"], sc, c)
        y = ops.rmsnorm_modulate(d["x"], d["w"], d["mod"], -1, sc)
        S.check_rmsnorm_modulate(y.cpu(), k["x"], k["w"], scale, None, what=f"rmsnorm_modulate (no shift) c{c}")
        x2 = d["x"].clone()
        x1, _ = ops.gated_residual_out(d["x"], d["r"], d["gmod"], c)
        assert torch.equal(ops.gated_residual_rmsnorm_modulate_(x2, d["r"], d["gmod"], c, d["w"], d["mod"], -1, sc), ops.rmsnorm_modulate(x1, d["w"], d["mod"], -1, sc))
        dmod = torch.full((b, 4 * c), 7.0, device=DEV)
        dx = d["dres"].clone()
        dw = ops.rmsnorm_modulate_bwd_(dx, d["da"], d["x"], d["w"], d["mod"], dmod, -1, sc)
        dm = dmod.cpu()
        S.check_rmsnorm_modulate_bwd(dx.cpu(), None, S.chunk(dm, sc, c), dw.cpu(), k["dres"], k["da"], k["x"], k["w"], scale, what=f"rmsnorm_modulate_bwd (no shift) c{c}")
        own = torch.zeros(4 * c, dtype=torch.bool)
        own[sc:sc + c] = True
        assert bool((dm[:, ~own] == 7.0).all()), "rmsnorm_modulate_bwd wrote a shift chunk that does not exist"


def _head_kw(k, norm, rope):
    return dict(qw=k["qw"] if norm else None, kw=k["kw"] if norm else None, cos=k["cos"] if rope else None, sin=k["sin"] if rope else None)


@pytest.mark.parametrize("norm,rope", [(False, True), (False, False), (True, False)])
@pytest.mark.parametrize("n", [5, 64])
@pytest.mark.parametrize("heads,d", [(3, 64), (2, 72), (2, 40)])
def test_head_split_forward_and_backward(heads, d, n, norm, rope):
    from dmvae_amd import ops
    k = S.qk_case(2, n, heads, d, seed=3)
    kw = _head_kw(k, norm, rope)
    dk_ = {a: (None if v is None else v.to(DEV)) for a, v in kw.items()}
    qkv = k["qkv"].to(DEV)
    q, kk, v = ops.head_split(qkv, heads, **dk_)
    assert q.shape == (2 * heads, n, k["dp"]) and v.shape == (2 * heads, n, d) and k["dp"] % 32 == 0
    V.check_head_split(q.cpu(), kk.cpu(), v.cpu(), k["qkv"], heads, what=f"head_split norm{norm} rope{rope}", **kw)
    dq, dk, dv = k["dq"].to(DEV), k["dk"].to(DEV), k["dv"].to(DEV)
    dqkv, dqw, dkw = ops.head_split_bwd(dq, dk, dv, qkv, heads, **dk_)
    cpu = lambda t: None if t is None else t.cpu()
    o = V.check_head_split_bwd(dqkv.cpu(), cpu(dqw), cpu(dkw), k["dq"], k["dk"], k["dv"], k["qkv"], heads, what=f"head_split_bwd norm{norm} rope{rope}", **kw)
    # ... which is autograd over the forward definition (straight through its rounding)
    x = k["qkv"].double().requires_grad_(True)
    qq, kq, _, _, vv = V.head_split(x, heads, rnd=True, **kw)
    ((qq * k["dq"][..., :d].double()).sum() + (kq * k["dk"][..., :d].double()).sum() + (vv * k["dv"].double()).sum()).backward()
    assert torch.allclose(o["dqkv"], x.grad, rtol=1e-10, atol=1e-10)
    # frozen norm weights: the same dqkv bits, no weight gradient
    dqkv2, a, b_ = ops.head_split_bwd(dq, dk, dv, qkv, heads, need_w=False, **dk_)
    assert a is None and b_ is None and torch.equal(dqkv2, dqkv)
    again = ops.head_split_bwd(dq, dk, dv, qkv, heads, **dk_)
    assert torch.equal(again[0], dqkv) and (dqw is None or (torch.equal(again[1], dqw) and torch.equal(again[2], dkw)))


def test_head_split_with_norm_and_rope_computes_what_qknorm_rope_computes():
    from dmvae_amd import ops
    k = S.qk_case(2, 64, 2, 72, seed=5)
    d = _dev(k)
    q, kk, v = ops.head_split(d["qkv"], 2, d["qw"], d["kw"], d["cos"], d["sin"])
    S.check_qknorm_rope(q.cpu(), kk.cpu(), v.cpu(), k["qkv"], k["qw"], k["kw"], k["cos"], k["sin"], 2, what="head_split (rms, rope)")


@pytest.mark.parametrize("n", [1, 7, 8 * 1024 + 3])
def test_gelu_tanh_forward_and_backward(n):
    from dmvae_amd import ops
    x = V.gelu_inputs(n)
    dy = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(BF)
    y = ops.gelu_tanh(x.to(DEV))
    V.check_gelu_tanh(y.cpu(), x)
    dx = ops.gelu_tanh_bwd(dy.to(DEV), x.to(DEV))
    V.check_gelu_tanh_bwd(dx.cpu(), dy, x)
    if n > 8:                                   # a view that starts off a 16-byte boundary: the element-wise path, the same bits
        buf = torch.empty(n + 8, dtype=BF, device=DEV)
        buf[1:n + 1] = x.to(DEV)
        view = buf[1:n + 1]
        assert view.data_ptr() % 16 != 0 and torch.equal(ops.gelu_tanh(view), y) and torch.equal(ops.gelu_tanh_bwd(dy.to(DEV), view), dx)


def test_gelu_tanh_special_values_as_torch():
    """+-0, the bf16 extremes, inf and NaN: the NaN / inf pattern and the signs of zero of torch's own tanh-GELU on the same device, forward and backward."""
    import torch.nn.functional as F
    from dmvae_amd import ops
    x = torch.tensor(V.GELU_SPECIALS, dtype=torch.float32).to(BF).to(DEV)
    y = ops.gelu_tanh(x)
    xr = x.clone().requires_grad_(True)
    ref = F.gelu(xr, approximate="tanh")
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(torch.isinf(y), torch.isinf(ref))
    fin = torch.isfinite(ref)
    assert torch.equal(y[fin].float(), ref[fin].float()) and torch.equal(torch.signbit(y[fin]), torch.signbit(ref[fin]))      # 0, -0, x itself at the large values
    dy = torch.ones_like(x)
    ref.backward(dy)
    dx = ops.gelu_tanh_bwd(dy, x)
    assert torch.equal(torch.isnan(dx), torch.isnan(xr.grad)) and torch.equal(torch.isinf(dx), torch.isinf(xr.grad))
    fin = torch.isfinite(xr.grad)
    assert torch.allclose(dx[fin].float(), xr.grad[fin].float(), rtol=2 ** -7, atol=1e-6)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def _load(tag):
    g = load_golden(tag)
    return g, V.build(tag, g).to(DEV), g.t("x"), g.t("t"), torch.from_numpy(np.asarray(g["y"]))


@functools.lru_cache(maxsize=None)
def _twin(tag):
    """The bf16-site restatement on the CPU, forward and autograd backward, computed once per fixture: (out, dx, {name: grad})."""
    g = load_golden(tag)
    m = V.build(tag, g)
    names = [n for n, _ in m.named_parameters()]
    po = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for n in names:
        po[n].requires_grad_(n != "pos_embed")
    xo = g.t("x").clone().requires_grad_(True)
    yo = V.lightningdit_forward(xo, g.t("t"), torch.from_numpy(np.asarray(g["y"])), po, V.CFGS[tag], q=Q)
    yo.backward(g.t("dy"))
    return yo.detach(), xo.grad.detach(), {n: po[n].grad.detach() for n in names if po[n].grad is not None}


def _count_new_ops(mp, counts):
    """Wraps the ops that only a variant reaches: the entry points of csrc/dit_variants.hip, and the RMSNorm kernels' no-shift form.  Also the default block's own
    head split (`qknorm_rope`, `qknorm_rope_bwd`: the per-block training route of every configuration with QK-norm and RoPE)."""
    from dmvae_amd import ops

    def wrap(name, key, is_hit=lambda a, kw: True):
        fn = getattr(ops, name)

        def counted(*a, **kw):
            if is_hit(a, kw):
                counts[key] = counts.get(key, 0) + 1
            return fn(*a, **kw)
        mp.setattr(ops, name, counted)
    for name in ("layernorm_modulate", "gated_residual_layernorm_modulate_", "gated_residual_layernorm_out", "layernorm_modulate_bwd_"):
        wrap(name, "layernorm_bwd" if name.endswith("bwd_") else "layernorm")
    wrap("head_split", "head_split")
    wrap("head_split_bwd", "head_split_bwd")
    wrap("gelu_tanh", "gelu_tanh")
    wrap("gelu_tanh_bwd", "gelu_tanh_bwd")
    wrap("rmsnorm_modulate", "no_shift", lambda a, kw: a[3] < 0)
    wrap("gated_residual_rmsnorm_modulate_", "no_shift", lambda a, kw: a[6] < 0)
    wrap("gated_residual_out", "no_shift", lambda a, kw: len(a) > 4 and a[4] is not None and a[6] < 0)
    wrap("rmsnorm_modulate_bwd_", "no_shift_bwd", lambda a, kw: a[6] < 0)
    wrap("qknorm_rope", "qknorm_rope")
    wrap("qknorm_rope_bwd", "qknorm_rope_bwd")


def _expected_new_ops(tag, grad):
    f = V.flags(V.CFGS[tag])
    want = set()
    if not f["use_rmsnorm"]:
        want |= {"layernorm"} | ({"layernorm_bwd"} if grad else set())
    if not (f["use_qknorm"] and f["use_rope"]):
        want |= {"head_split"} | ({"head_split_bwd"} if grad else set())
    if not f["use_swiglu"]:
        want |= {"gelu_tanh"} | ({"gelu_tanh_bwd"} if grad else set())
    if f["wo_shift"] and f["use_rmsnorm"]:
        want |= {"no_shift"} | ({"no_shift_bwd"} if grad else set())
    return want


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("tag", TAGS)
def test_variant_runs_on_the_kernels_without_the_stock_opt_in(tag, grad, monkeypatch):
    """Before the variant route every one of these raised DmvaeHipError (DMVAE_ALLOW_STOCK unset).  Now the call returns, the variant's own kernels are launched and
    `forward_stock` is never entered."""
    from dmvae_amd.models.lightningdit import LightningDiT
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    g, m, x, t, y = _load(tag)

    def no_stock(*a, **kw):
        raise AssertionError("forward_stock entered")
    monkeypatch.setattr(LightningDiT, "forward_stock", no_stock)
    counts = {}
    _count_new_ops(monkeypatch, counts)
    if grad:
        xa = x.to(DEV).requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            out = m(xa, t.to(DEV), y.to(DEV))
        (out.float() * g.t("dy").to(DEV)).sum().backward()
        assert xa.grad is not None and torch.isfinite(xa.grad).all()
    else:
        m.requires_grad_(False)
        with torch.autocast("cuda", dtype=BF):
            out = m(x.to(DEV), t.to(DEV), y.to(DEV))
        assert not out.requires_grad
    assert out.dtype == BF and out.shape == x.shape and torch.isfinite(out).all()
    want = _expected_new_ops(tag, grad)
    assert want and want <= {k for k, v in counts.items() if v > 0}, (want, counts)


@pytest.mark.parametrize("tag", TAGS)
def test_variant_inference_vs_capture_spec_and_stock(tag):
    g, m, x, t, y = _load(tag)
    m.requires_grad_(False)
    xd, td, yd = x.to(DEV), t.to(DEV), y.to(DEV)
    with torch.autocast("cuda", dtype=BF):
        out = m(xd, td, yd)                                                       # lightningdit_fast.forward_inference
        ref_stock = m.forward_stock(xd, td, yd)
    assert out.dtype == BF and out.shape == x.shape
    yo = _twin(tag)[0]
    e_fast, e_stock, e_orc = _rl2(out.float().cpu(), g.t("out")), _rl2(ref_stock.float().cpu(), g.t("out")), _rl2(yo, g.t("out"))
    print(f"{tag}: rel-L2 to the f32 reference -- HIP path {e_fast:.2e}, stock autocast {e_stock:.2e}, bf16-site spec {e_orc:.2e}; HIP to spec {_rl2(out.float().cpu(), yo):.2e}")
    assert _rl2(out.float().cpu(), yo) < 2e-2                                    # same rounding sites, different accumulation order
    assert e_fast < 1.5 * max(e_stock, e_orc) + 2e-3                              # as close to the f32 reference as the reference's own autocast run
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        assert torch.equal(m(xd, td, yd), out)                                    # reruns bit-identical


@pytest.mark.parametrize("tag", TAGS)
def test_variant_train_route_vs_reference_capture_by_the_bf16_site_criterion(tag):
    """test_gpu_dit.py's criterion for the default block, with autograd over the variant restatement as the twin: as close to the reference's f32 capture as the
    CPU run with bf16 rounding at exactly the autocast sites is (x 1.15 + 1e-3; gradient norms x 1.15 + 1e-2)."""
    g, m, x, t, y = _load(tag)
    dy = g.t("dy")
    f = V.flags(V.CFGS[tag])

    def run(model, x_req=True):
        xa = x.to(DEV).requires_grad_(x_req)
        with torch.autocast("cuda", dtype=BF):
            out = model(xa, t.to(DEV), y.to(DEV))
        (out.float() * dy.to(DEV)).sum().backward()
        return out, xa
    out, xa = run(m)
    yo, dxo, go = _twin(tag)

    def floor(hip, orc, ref, what, slack=1.15, abs_floor=1e-3):
        e_hip, e_orc = _rl2(hip, ref), _rl2(orc, ref)
        print(f"{tag} {what}: rel-L2 to the f32 reference -- HIP {e_hip:.2e}, bf16-site spec {e_orc:.2e}")
        assert e_hip < slack * e_orc + abs_floor, (what, e_hip, e_orc)
    floor(out.float().cpu(), yo, g.t("out"), "out")
    floor(xa.grad.cpu(), dxo, g.t("dx"), "dx")
    pa = dict(m.named_parameters())
    full = [k[2:] for k in g.keys() if k.startswith("g.")]
    assert len(full) == 6
    for n in full:
        floor(pa[n].grad.cpu(), go[n], g.t("g." + n), "grad " + n)
    for n, p in pa.items():                 # EVERY parameter: gradient norm against the reference's, to the twin's own distance
        if n == "pos_embed":
            assert p.grad is None
            continue
        assert p.grad is not None and "gn." + n in g, n
        want_norm = float(g["gn." + n][0])
        if want_norm < 1e-3:
            continue
        e_hip = abs(p.grad.double().norm().item() - want_norm) / want_norm
        e_orc = abs(go[n].double().norm().item() - want_norm) / want_norm
        assert e_hip < 1.15 * e_orc + 1e-2, (n, e_hip, e_orc)
    # absent parameters have no entry on either side; the adaLN row has the configuration's width
    assert {k[3:] for k in g if k.startswith("gn.")} == {n for n, p in pa.items() if p.grad is not None}
    assert ("blocks.0.attn.q_norm.weight" in pa) == f["use_qknorm"] and ("blocks.0.norm1.weight" in pa) == f["use_rmsnorm"]
    c = V.CFGS[tag]["hidden_size"]
    assert pa["blocks.0.adaLN_modulation.1.weight"].grad.shape == ((4 if f["wo_shift"] else 6) * c, c)
    assert pa["blocks.1.adaLN_modulation.1.bias"].grad.shape == ((4 if f["wo_shift"] else 6) * c,)
    # two runs are bit-identical
    keep = {n: p.grad.clone() for n, p in pa.items() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    out2, xb = run(m)
    assert torch.equal(out2, out) and torch.equal(xb.grad, xa.grad)
    assert all(torch.equal(pa[n].grad, v) for n, v in keep.items())
    # frozen weights, gradient for the input only (the likelihood sampler's VJP): the same output and the same dx, no parameter gradient
    m.zero_grad(set_to_none=True)
    m.requires_grad_(False)
    out3, xc = run(m)
    assert torch.equal(out3, out) and torch.equal(xc.grad, xa.grad)
    assert all(p.grad is None for p in m.parameters())


def test_plain_variant_above_288_tokens_streams_its_attention(monkeypatch):
    """576 tokens at head dim 64: the head split feeds the streaming attention kernels, forward and backward; against the stock modules under autocast at
    test_gpu_dit.py::test_lightningdit_train_route_matches_stock_autocast's bounds."""
    import copy
    from dmvae_amd import ops
    from dmvae_amd.models.lightningdit import LightningDiT
    from oracle.detweights import det_fill_
    cfg = dict(V.CFGS["dit_var_plain"], input_size=24, hidden_size=128, num_heads=2, depth=1)
    m = det_fill_(LightningDiT(**cfg).eval(), 86, skip=("pos_embed",)).to(DEV)
    ref = copy.deepcopy(m)
    gen = torch.Generator().manual_seed(86)
    x = torch.randn(1, 8, 24, 24, generator=gen).to(DEV)
    t, y = torch.rand(1, generator=gen).to(DEV), torch.tensor([3], device=DEV)
    dy = torch.randn(1, 8, 24, 24, generator=gen).to(DEV)
    counts = {}
    for name in ("attention_heads_stream", "attention_bwd_heads_stream"):
        fn = getattr(ops, name)

        def counted(*a, _fn=fn, _name=name, **kw):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        inf = m(x, t, y)
    assert counts.get("attention_heads_stream") == 1 and "attention_bwd_heads_stream" not in counts
    xa = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        out = m(xa, t, y)
    (out.float() * dy).sum().backward()
    assert counts.get("attention_heads_stream") == 2 and counts.get("attention_bwd_heads_stream") == 1
    xb = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        outs = ref.forward_stock(xb, t, y)
    (outs.float() * dy).sum().backward()
    assert _rl2(out.float(), outs.float()) < 1e-2 and _rl2(inf.float(), outs.float()) < 1e-2
    assert _rl2(xa.grad, xb.grad) < 3e-2
    pb = dict(ref.named_parameters())
    for n_, p in m.named_parameters():
        if n_ == "pos_embed":
            continue
        assert p.grad is not None, n_
        assert _rl2(p.grad, pb[n_].grad) < 4e-2, (n_, _rl2(p.grad, pb[n_].grad))


# ---- one block Function (`functional.DitBlockFn`) for the default and the variant blocks ---------------------------------------------------
def _frozen_case(shape, config):
    """A depth-2 model of dit_variants_spec.FROZEN_SHAPES x FROZEN_CONFIGS with deterministic non-zero weights, and B = 2 inputs."""
    from dmvae_amd.models import lightningdit_fast as LF
    from dmvae_amd.models.lightningdit import LightningDiT
    from oracle.detweights import det_fill_
    cfg = V.frozen_case_cfg(shape)
    m = det_fill_(LightningDiT(**cfg, **V.FROZEN_CONFIGS[config]).eval(), 91, skip=("pos_embed",)).to(DEV)
    assert LF.structurally_supported(m) if config == "default" else LF.variant_supported(m)
    side = cfg["input_size"]
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(2, 16, side, side, generator=gen).to(DEV)
    t, y = torch.rand(2, generator=gen).to(DEV), torch.tensor([3, 7], device=DEV)
    dy = torch.randn(2, 16, side, side, generator=gen).to(DEV)
    return m, x, t, y, dy


def _fwd_bwd(m, x, t, y, dy, before_backward=lambda: None):
    m.zero_grad(set_to_none=True)
    xa = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        out = m(xa, t, y)
    before_backward()
    (out.float() * dy).sum().backward()
    return out.detach(), xa.grad


def test_default_block_reaches_no_variant_kernel(monkeypatch):
    """The default model on the per-block route (`STACK_FN` False: `DitBlockFn`, the Function the variants share) and on the stack route: no entry point of
    csrc/dit_variants.hip and no no-shift launch, forward or backward; per block its own `qknorm_rope` / `qknorm_rope_bwd`, never `head_split`."""
    from dmvae_amd.models import lightningdit_fast as LF
    m, x, t, y, dy = _frozen_case("resident", "default")
    for stack in (False, True):
        counts = {}
        with monkeypatch.context() as mp:
            mp.setattr(LF, "STACK_FN", stack)
            _count_new_ops(mp, counts)
            out, dx = _fwd_bwd(m, x, t, y, dy)
        assert out.float().abs().max() > 0 and dx.abs().max() > 0
        own = {k: counts.pop(k, 0) for k in ("qknorm_rope", "qknorm_rope_bwd")}
        assert not any(counts.values()), (stack, counts)
        if not stack:
            assert own["qknorm_rope"] == len(m.blocks) and own["qknorm_rope_bwd"] == len(m.blocks), own


@pytest.mark.parametrize("config", list(V.FROZEN_CONFIGS))
@pytest.mark.parametrize("shape", list(V.FROZEN_SHAPES))
def test_frozen_and_trainable_runs_give_the_same_input_gradient_bits(shape, config, monkeypatch):
    """`DitBlockFn` with no parameter needing a gradient (`need_w` False: dx-only Linear backward, no norm-weight sums) against the same model trainable: the same
    output and the same d x bit for bit, no parameter gradient -- in each attention regime (resident, streaming with lse, composed with the saved P) and for the
    default block (per-block route), the default without QK-norm, and LayerNorm + GELU-MLP + `wo_shift` without QK-norm."""
    from dmvae_amd.models import lightningdit_fast as LF
    monkeypatch.setattr(LF, "STACK_FN", False)
    m, x, t, y, dy = _frozen_case(shape, config)
    out, dx = _fwd_bwd(m, x, t, y, dy)
    assert out.float().abs().max() > 0 and dx.abs().max() > 0
    assert all(p.grad is not None for n, p in m.named_parameters() if n != "pos_embed")
    m.requires_grad_(False)
    out_f, dx_f = _fwd_bwd(m, x, t, y, dy)
    assert torch.equal(out_f, out) and torch.equal(dx_f, dx)
    assert all(p.grad is None for p in m.parameters())


def test_frozen_default_block_does_no_weight_gradient_work(monkeypatch):
    """The frozen default model on the per-block route: its backward reaches none of the weight-gradient entry points (before the default block shared the variants'
    Function it computed every weight gradient and dropped it)."""
    from dmvae_amd import ops
    from dmvae_amd.models import lightningdit_fast as LF
    monkeypatch.setattr(LF, "STACK_FN", False)
    m, x, t, y, dy = _frozen_case("resident", "default")
    m.requires_grad_(False)
    calls = []

    def watch():
        for name in ("conv2d_nhwc_wgrad", "linear_wgrad_grouped", "linear_rows_wgrad"):
            fn = getattr(ops, name)
            monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _name=name, **kw: (calls.append(_name), _fn(*a, **kw))[1])
    out, dx = _fwd_bwd(m, x, t, y, dy, before_backward=watch)
    assert dx.abs().max() > 0 and not calls, calls
    assert all(p.grad is None for p in m.parameters())


# ---- riders: what sits above `forward` works for a variant with no code of its own ----------------------------------------------------------
def test_forward_with_cfg_equals_the_composition():
    g, m, x, t, y = _load("dit_var_plain")
    m.requires_grad_(False)
    x2 = torch.cat([x, x]).to(DEV)
    t2 = torch.cat([t, t]).to(DEV)
    y2 = torch.cat([y, torch.full_like(y, 10)]).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        assert m._takes_inference_route(x2)
        a = m.forward_with_cfg(x2, t2, y2, 2.5)
        b = m.forward_with_cfg_composed(x2, t2, y2, 2.5)
        c = m.forward_with_cfg(x2, t2, y2, 1.5, cfg_interval=True, cfg_interval_start=0.0, standard_cfg=True)
        d = m.forward_with_cfg_composed(x2, t2, y2, 1.5, cfg_interval=True, cfg_interval_start=0.0, standard_cfg=True)
    assert torch.equal(a, b) and torch.equal(c, d)


@pytest.mark.parametrize("tag", ["dit_var_mix_a", "dit_var_mix_b"])
def test_a_2b_call_equals_two_b_calls(tag):
    from dmvae_amd.train import _batchable
    g, m, x, t, y = _load(tag)
    m.requires_grad_(False)
    x, t, y = x.to(DEV), t.to(DEV), y.to(DEV)
    null = torch.full_like(y, 10)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        vc, vu = m(x, t, y), m(x, t, null)
        v2 = m(torch.cat([x, x]), torch.cat([t, t]), torch.cat([y, null]))
    b = x.shape[0]
    assert torch.equal(v2[:b], vc) and torch.equal(v2[b:], vu) and not torch.equal(vc, vu)
    assert _batchable(m.eval()) and not _batchable(m.train())


def test_graphed_inference_replays_to_the_eager_bits():
    from dmvae_amd.models.lightningdit_fast import GraphedInference
    g, m, x, t, y = _load("dit_var_mix_a")
    m.requires_grad_(False)
    x, t, y = x.to(DEV), t.to(DEV), y.to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        eager = m(x, t, y)
        gi = GraphedInference(m, x, t, y)
        assert torch.equal(gi(x, t, y), eager)
        x2 = x.flip(0).contiguous()
        want = m(x2, t, y)
        assert torch.equal(gi(x2, t, y), want) and not torch.equal(want, eager)


def test_layernorm_qknorm_still_raises_and_names_the_combination(monkeypatch):
    from dmvae_amd._lib import DmvaeHipError
    from dmvae_amd.models.lightningdit import LightningDiT
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    m = LightningDiT(**V.CFG_LAYERNORM_QK).eval().to(DEV)
    x = torch.zeros(1, 8, 8, 8, device=DEV)
    with torch.autocast("cuda", dtype=BF), pytest.raises(DmvaeHipError) as ei:
        m(x, torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV))
    msg = str(ei.value)
    assert "use_qknorm=True" in msg and "use_rmsnorm=False" in msg and "LayerNorm" in msg
