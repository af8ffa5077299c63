"""The kernels under the DINOv2 discriminator (models/dinodisc.py of the reference; --disc_type dino) on an MI355X (-m gpu), each against float64 on its OWN
operands: the LayerNorm family at ViT-S's width 384 (csrc/vit.hip, csrc/vit_bwd.hip), the convolution along the token axis (csrc/conv_tokens.hip: forward,
input gradient, weight + bias gradient, the weight pack) and BatchNormLocal + LeakyReLU through the GroupNorm entry points (virtual groups as "images", one
channel per group).

Bars (none is taken from what the kernels give):
  LayerNorm 384       those the same kernels are held to at width 256 / 1024: test_gpu_train_step.py (plain: RNE(f64) or |err| < 2e-2, and
                      |err| / (|ref| + 1) < 5e-3), test_gpu_vit_pin.py (fused: the two kernels' bits, and max |err| / max |ref| < 2^-8),
                      test_gpu_vit_train.py (backward: dx 2e-6, dgamma / dbeta 1e-5 rel_err, reruns bit-identical, accumulate)
  token conv, bf16    every element a correct rounding of the f64 value: test_gpu_modules._assert_bf16_of (<= 1 bf16 spacing, != RNE(f64) for <= 0.2 %)
  token conv, f32     rel_err < 1e-5 (the weight-gradient bar of test_gpu_modules.py)
  BatchNormLocal      test_gpu_batchnorm_kernels.py's: statistics 1e-5 relative (the mean: of |mean| + std of its channel), bf16 outputs |err| <= 2^-8 |ref| + 1e-5 max |ref|, dgamma / dbeta rel_err 1e-5;
                      da is zeroed where the f64 pre-activation has |u| < 1e-3 (LeakyReLU's side is not decidable in f32 there), as that file does
  module              the bf16-site criterion, stated in front of the module tests below

Figures observed on an MI355X (module tests; rel-L2 to the reference's f32 capture, HIP route / CPU twin):
  train logits 9.62e-3 / 9.62e-3; the 16 head gradients: ratio HIP / twin 0.86 ... 1.06 (errors 6.8e-3 ... 7.8e-2); the last biases' gradients 4.8e-7 and 6.6e-8 [1e-5];
  zero-gradient conv biases max |grad| 2.2e-2 ... 3.3e-2 (twin 1.9e-2 ... 3.7e-2) [bounds 3.6 ... 7.5]; eval logits 9.88e-3 / 9.70e-3; dx 7.26e-2 / 7.37e-2;
  branches crop 6.84e-3 / 6.62e-3, 252 px 6.72e-3 / 6.72e-3, 70 px 6.24e-3 / 6.71e-3
"""
import functools
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SLOPE = float(np.float32(0.2))


def _ops():
    from dmvae_amd import ops
    return ops


# ---- LayerNorm family at width 384 -------------------------------------------------------------------------------------------------------------------------
LN_ROWS = [1, 7, 650]


@functools.lru_cache(maxsize=None)
def _ln_inputs(rows):
    g = torch.Generator().manual_seed(384 + rows)
    x = torch.randn(rows, 384, generator=g) * 2 + 0.3
    r = torch.randn(rows, 384, generator=g).to(BF)
    ls = torch.randn(384, generator=g) * 0.1
    gam, bet = 1 + 0.3 * torch.randn(384, generator=g), torch.randn(384, generator=g)
    dy = torch.randn(rows, 384, generator=g).to(BF)
    dres = torch.randn(rows, 384, generator=g)
    return x, r, ls, gam, bet, dy, dres


@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_384(rows):
    ops = _ops()
    x, _, _, gam, bet, _, _ = (t.to(DEV) for t in _ln_inputs(rows))
    y = ops.layernorm_bf16(x, gam, bet, 1e-6)
    ref = F.layer_norm(x.double(), (384,), gam.double(), bet.double(), 1e-6)
    assert torch.equal(y, ref.float().to(BF)) or (y.float() - ref.float()).abs().max() < 2e-2
    assert ((y.double() - ref).abs() / (ref.abs() + 1)).max() < 5e-3
    assert torch.equal(y, ops.layernorm_bf16(x, gam, bet, 1e-6))


@pytest.mark.parametrize("rows", LN_ROWS)
def test_scale_residual_layernorm_384(rows):
    ops = _ops()
    x, r, ls, gam, bet, _, _ = (t.to(DEV) for t in _ln_inputs(rows))
    x1 = x.clone()
    y1 = ops.scale_residual_layernorm_(x1, r, ls, gam, bet, 1e-6)
    x2 = ops.scale_residual_(x.clone(), r, ls)
    y2 = ops.layernorm_bf16(x2, gam, bet, 1e-6)
    assert torch.equal(x1, x2) and torch.equal(y1, y2)
    xr = x.double() + ls.double() * r.double()
    yr = F.layer_norm(xr, (384,), gam.double(), bet.double(), 1e-6)
    assert (x1.double() - xr).abs().max() < 1e-5
    assert ((y1.double() - yr).abs().max() / yr.abs().max()).item() < 2.0 ** -8


@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_bwd_384(rows):
    ops = _ops()
    x, _, _, gam, bet, dy, dres = (t.to(DEV) for t in _ln_inputs(rows))
    xr = x.double().requires_grad_(True)
    gr, br = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    F.layer_norm(xr, (384,), gr, br, 1e-6).backward(dy.double())
    dx = dres.clone()
    dg, db = ops.layernorm_bwd_(dx, dy, x, gam, 1e-6)
    assert rel_err(dx, dres.double() + xr.grad) < 2e-6
    assert rel_err(dg, gr.grad) < 1e-5 and rel_err(db, br.grad) < 1e-5
    dx2 = dres.clone()
    dg2, db2 = ops.layernorm_bwd_(dx2, dy, x, gam, 1e-6)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    acc_g, acc_b = dg.clone(), db.clone()
    ops.layernorm_bwd_(dres.clone(), dy, x, gam, 1e-6, dg_out=acc_g, db_out=acc_b, accumulate=True)
    assert rel_err(acc_g, 2 * gr.grad) < 1e-5 and rel_err(acc_b, 2 * br.grad) < 1e-5
    dx3 = dres.clone()                                   # the frozen backbone's form: no parameter gradients, the same dx
    assert ops.layernorm_bwd_(dx3, dy, x, gam, 1e-6, need_param_grads=False) == (None, None)
    assert torch.equal(dx3, dx)


# ---- convolution along the token axis ----------------------------------------------------------------------------------------------------------------------
CONV_CASES = [(1, 5, 384, 9),       # fewer tokens than the taps reach on either side
              (3, 25, 384, 9),      # the 70 px grid: every token sees padding on one side or both
              (2, 324, 384, 9),     # the production grid (18 x 18): six token tiles, the last one ragged
              (2, 324, 384, 1)]     # the degenerate kernel size


@functools.lru_cache(maxsize=None)
def _conv_case(b, l, c, ks):
    """CPU operands and the f64 results on them; shared by the tests of a shape, never written to.  The weight the f64 side uses is the bf16 pack the kernels
    read (checked bit for bit against its definition in test_conv_tokens_pack)."""
    g = torch.Generator().manual_seed(1000 * l + 10 * ks + b)
    x = torch.randn(b, l, c, generator=g).to(BF)
    dy = torch.randn(b, l, c, generator=g).to(BF)
    w = torch.randn(c, c, ks, generator=g) * (c * ks) ** -0.5 * 1.7
    bias = 0.1 * torch.randn(c, generator=g)
    sigma = torch.tensor([1.7])
    wq = (w / sigma).to(BF)                                                # [co, ci, t]
    x64 = x.double().transpose(1, 2).requires_grad_(True)                  # [B, C, L], the reference's layout
    w64, b64 = wq.double().requires_grad_(True), bias.double().requires_grad_(True)
    y = F.conv1d(x64, w64, b64, padding=ks // 2)
    y.backward(dy.double().transpose(1, 2))
    return dict(x=x, dy=dy, w=w, bias=bias, sigma=sigma, wq=wq, y=y.detach().transpose(1, 2).contiguous(), dx=x64.grad.transpose(1, 2).contiguous(),
                dw=w64.grad, db=b64.grad)


def _packs(case):
    return _ops().conv_tokens_pack(case["w"].to(DEV), case["sigma"].to(DEV))


@pytest.mark.parametrize("ks", [1, 9])
def test_conv_tokens_pack(ks):
    """Both packs are the bf16 rounding of w / sigma (an f32 division), laid out [C_out][ks][C_in] and [C_in][ks reversed][C_out]; sigma = NULL is 1."""
    case = _conv_case(2, 324, 384, ks)
    wf, wd = _packs(case)
    wq = case["wq"].to(DEV)
    assert torch.equal(wf, wq.permute(0, 2, 1).contiguous())
    assert torch.equal(wd, wq.flip(2).permute(1, 2, 0).contiguous())
    wf1, _ = _ops().conv_tokens_pack(case["w"].to(DEV))
    assert torch.equal(wf1, case["w"].to(DEV).to(BF).permute(0, 2, 1).contiguous())


@pytest.mark.parametrize("b,l,c,ks", CONV_CASES)
def test_conv_tokens_fwd_and_dgrad(b, l, c, ks):
    from test_gpu_modules import _assert_bf16_of
    ops = _ops()
    case = _conv_case(b, l, c, ks)
    wf, wd = _packs(case)
    x, dy, bias = case["x"].to(DEV), case["dy"].to(DEV), case["bias"].to(DEV)
    y = ops.conv_tokens(x, wf, bias)
    _assert_bf16_of(y, case["y"], f"conv_tokens {b, l, c, ks}")
    dx = ops.conv_tokens_dgrad(dy, wd)
    _assert_bf16_of(dx, case["dx"], f"conv_tokens_dgrad {b, l, c, ks}")
    assert torch.equal(y, ops.conv_tokens(x, wf, bias)) and torch.equal(dx, ops.conv_tokens_dgrad(dy, wd))
    y0 = ops.conv_tokens(x, wf)                                            # no bias
    _assert_bf16_of(y0, case["y"] - case["bias"].double(), f"conv_tokens without bias {b, l, c, ks}")


@pytest.mark.parametrize("b,l,c,ks", CONV_CASES)
def test_conv_tokens_wgrad(b, l, c, ks):
    ops = _ops()
    case = _conv_case(b, l, c, ks)
    x, dy = case["x"].to(DEV), case["dy"].to(DEV)
    dw, db = ops.conv_tokens_wgrad(dy, x, ks)
    assert dw.shape == (c, c, ks) and dw.dtype == torch.float32
    assert rel_err(dw.cpu(), case["dw"]) < 1e-5
    assert rel_err(db.cpu(), case["db"]) < 1e-5
    dw2, db2 = ops.conv_tokens_wgrad(dy, x, ks)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    dw3, none = ops.conv_tokens_wgrad(dy, x, ks, need_bias=False)
    assert none is None and torch.equal(dw3, dw)


def test_conv_tokens_does_not_depend_on_the_batch():
    """Forward and input gradient at batch 4 are the bits of two batch-2 calls."""
    ops = _ops()
    case = _conv_case(2, 324, 384, 9)
    wf, wd = _packs(case)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 324, 384, generator=g).to(BF).to(DEV)
    y = ops.conv_tokens(x, wf, case["bias"].to(DEV))
    assert torch.equal(y, torch.cat([ops.conv_tokens(x[:2].contiguous(), wf, case["bias"].to(DEV)), ops.conv_tokens(x[2:].contiguous(), wf, case["bias"].to(DEV))]))
    dx = ops.conv_tokens_dgrad(x, wd)
    assert torch.equal(dx, torch.cat([ops.conv_tokens_dgrad(x[:2].contiguous(), wd), ops.conv_tokens_dgrad(x[2:].contiguous(), wd)]))


def test_conv_tokens_refuses_what_it_does_not_cover():
    from dmvae_amd._lib import DmvaeHipError
    ops = _ops()
    x = torch.zeros(1, 4, 256, dtype=BF, device=DEV)
    with pytest.raises(DmvaeHipError, match="multiple of 32 in 384"):
        ops.conv_tokens(x, torch.zeros(256, 3, 256, dtype=BF, device=DEV))
    x = torch.zeros(1, 4, 384, dtype=BF, device=DEV)
    with pytest.raises(DmvaeHipError, match="ks odd"):
        ops.conv_tokens(x, torch.zeros(384, 4, 384, dtype=BF, device=DEV))


# ---- BatchNormLocal + LeakyReLU through the GroupNorm entry points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups_v,per,l", [(2, 6, 25), (1, 2, 324)])
def test_batchnorm_local_leaky(groups_v, per, l):
    """BatchNormLocal (models/dinodisc.py:29-56) on token-major [B, L, C]: G = `groups_v` virtual groups of `per` samples, statistics per (group, channel) over
    samples x tokens, biased variance, eps 1e-6 inside the sqrt -- the GroupNorm kernels with n = G "images" of per * L rows and one channel per group."""
    ops = _ops()
    c, eps = 384, float(np.float32(1e-6))
    g = torch.Generator().manual_seed(groups_v * 100 + per)
    mu, sd = torch.rand(c, generator=g) * 6 - 3, torch.rand(c, generator=g) * 1.8 + 0.2
    x = (torch.randn(groups_v * per, l, c, generator=g) * sd + mu).to(BF)
    gamma, beta = 1 + 0.5 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    da = torch.randn(groups_v * per, l, c, generator=g).to(BF)
    assert _lib().dmvae_groupnorm_workspace(groups_v, per * l, c, c) > 0
    x64 = x.double().view(groups_v, per * l, c).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean, var = x64.mean(1, keepdim=True), x64.var(1, unbiased=False, keepdim=True)
    u = (x64 - mean) / torch.sqrt(var + eps) * g64 + b64
    amb = u.detach().abs() < 1e-3
    assert amb.double().mean().item() < 5e-3
    da_used = da.view(groups_v, per * l, c).masked_fill(amb, 0)
    yr = F.leaky_relu(u, SLOPE)
    yr.backward(da_used.double())
    xd, dad = x.to(DEV).view(groups_v, per * l, c), da_used.to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    st = ops.groupnorm_stats(xd, c, eps)
    scale = mean.detach()[:, 0].abs() + var.detach()[:, 0].sqrt()            # an f32 sum's error scales with its terms: |mean| + std of the channel
    assert ((st[..., 0].cpu().double() - mean.detach()[:, 0]).abs() <= 1e-5 * scale).all()
    rstd = 1 / torch.sqrt(var.detach()[:, 0] + eps)
    assert ((st[..., 1].cpu().double() - rstd).abs() <= 1e-5 * rstd).all()

    def bf16_bar(got, ref):
        ref = ref.detach()
        return ((got.double().cpu() - ref).abs() / (2.0 ** -8 * ref.abs() + 1e-5 * ref.abs().max())).max().item()

    y = ops.groupnorm_apply(xd, st, gd, bd, 2, groups=c)
    assert bf16_bar(y, yr) <= 1.0
    dx, dg, db = ops.groupnorm_bwd(dad, xd, st, gd, bd, 2, groups=c)
    assert bf16_bar(dx, x64.grad) <= 1.0
    assert rel_err(dg.cpu(), g64.grad) < 1e-5 and rel_err(db.cpu(), b64.grad) < 1e-5
    dx2, none_g, none_b = ops.groupnorm_bwd(dad, xd, st, gd, bd, 2, groups=c, need_param_grads=False)
    assert none_g is None and none_b is None and torch.equal(dx2, dx)


def _lib():
    from dmvae_amd import _lib as L
    return L.lib()


# ---- the tap and the head tail ----------------------------------------------------------------------------------------------------------------------------------
def test_tap_and_untap():
    from test_gpu_modules import _assert_bf16_of
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    t = torch.randn(3, 26, 384, generator=g) * 2
    act = ops.dino_tap(t.to(DEV))
    _assert_bf16_of(act, t[:, 1:].double() + t[:, :1].double(), "tap", max_flip_frac=0.0)          # one f32 add of two f32 values, one rounding
    dact = torch.randn(3, 25, 384, generator=g).to(BF)
    dt = ops.dino_untap(dact.to(DEV))
    assert torch.equal(dt[:, 1:].cpu(), dact.float())
    assert rel_err(dt[:, 0].cpu(), dact.double().sum(1)) < 1e-6
    assert torch.equal(dt, ops.dino_untap(dact.to(DEV)))


@pytest.mark.parametrize("rows_shape", [(1, 5), (3, 25), (7, 324)])
def test_head_tail(rows_shape):
    from test_gpu_modules import _assert_bf16_of
    ops = _ops()
    c = 384
    g = torch.Generator().manual_seed(sum(rows_shape))
    a, h = torch.randn(*rows_shape, c, generator=g).to(BF), torch.randn(*rows_shape, c, generator=g).to(BF)
    w, bias = torch.randn(c, generator=g) * c ** -0.5, torch.randn(1, generator=g)
    dlogit = torch.randn(*rows_shape, generator=g)
    a64, h64, w64, b64 = (v.double().requires_grad_(True) for v in (a, h, w, bias))
    ref = ((a64 + h64) / np.sqrt(2) * w64).sum(-1) + b64
    ref.backward(dlogit.double())
    ad, hd, wd, bd = a.to(DEV), h.to(DEV), w.to(DEV), bias.to(DEV)
    logit = ops.dino_tail(ad, hd, wd, bd)
    assert logit.dtype == torch.float32 and rel_err(logit.cpu(), ref.detach()) < 1e-5
    dah, dw, db = ops.dino_tail_bwd(dlogit.to(DEV), ad, hd, wd)
    _assert_bf16_of(dah, a64.grad, "tail d a")
    assert torch.equal(a64.grad, h64.grad)
    assert rel_err(dw.cpu(), w64.grad) < 1e-5 and rel_err(db.cpu(), b64.grad) < 1e-5
    dah2, dw2, db2 = ops.dino_tail_bwd(dlogit.to(DEV), ad, hd, wd)
    assert torch.equal(dah, dah2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    dah3, none_w, none_b = ops.dino_tail_bwd(dlogit.to(DEV), ad, hd, wd, need_w=False)      # frozen heads
    assert none_w is None and none_b is None and torch.equal(dah3, dah)


# ---- the module by the bf16-site criterion -------------------------------------------------------------------------------------------------------------------
# rel-L2 to the reference's f32 capture no more than 1.15 x that of the CPU twin with bf16 rounding at the HIP route's storage sites (tests/dinodisc_spec.py).
# Where the twin itself sits at f32 rounding level (below 1e-5: quantities no bf16 site touches, such as the last bias' gradient = sum dy, which the twin's
# torch.sum reproduces to the bit) a ratio of two rounding noises says nothing and the HIP value is held to the f32 bar 1e-5 instead.
# The two conv biases in front of a BatchNormLocal have an analytically zero gradient (tests/test_dinodisc_cpu.py): bounded absolutely by 2^-8 (one bf16
# spacing) of the same conv's weight-gradient norm -- the bias gradient is the weight gradient of an all-ones input channel, whose entries a bf16-rounded
# activation gradient perturbs by 2^-9 of their terms; a channel's terms are far below the norm of the whole 384 x 384 (x 9) tensor.
F32_LEVEL = 1e-5
ZERO_GRAD_FACTOR = 2.0 ** -8


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _criterion(what, hip, twin, ref):
    e_hip, e_twin = _rel_l2(hip, ref), _rel_l2(twin, ref)
    print(f"[fig] {what}: rel-L2 to the f32 capture -- HIP {e_hip:.3e}, twin {e_twin:.3e}, ratio {e_hip / max(e_twin, 1e-30):.3f}")
    assert (e_hip <= 1.15 * e_twin) if e_twin >= F32_LEVEL else (e_hip < F32_LEVEL), (what, e_hip, e_twin)


def _sliced(k, v):
    return v.flatten()[::(97 if v.numel() < 200000 else 997)] if v.numel() >= 4096 else v


@functools.lru_cache(maxsize=None)
def _small_twin():
    """The capture and the twin's results on it (CPU, bf16 sites), computed once."""
    import dinodisc_spec as S
    from conftest import load_golden
    from oracle import ref_cpu as R
    g, c = load_golden("dinodisc_small"), S.SMALL
    _, backbone, heads = S.build_module()
    x = S.image(c["batch"], c["px"], c["x_seed"])
    dy = torch.randn(12, 648, generator=torch.Generator().manual_seed(c["dy_seed"]))
    p = {k: v.clone().requires_grad_(not k.endswith(("weight_u", "weight_v"))) for k, v in heads.items()}
    lt = S.forward(x, backbone, p, c["ks"], c["key_depths"], train=True, q=R.bf16_round)
    (lt * dy).sum().backward()
    xe = x.clone().requires_grad_(True)
    le = S.forward(xe, backbone, heads, c["ks"], c["key_depths"], train=False, q=R.bf16_round)
    (le * dy).sum().backward()
    return dict(g=g, x=x, dy=dy, logits_train=lt.detach(), grads={k: v.grad for k, v in p.items() if v.requires_grad}, logits_eval=le.detach(), dx=xe.grad)


@pytest.fixture
def hip_only(monkeypatch):
    """The route under test is the HIP route: no opt-in to the stock modules, and the stock functionals raise."""
    _small_twin()                                                    # the CPU twin uses the stock functionals: computed (once) before they are shut
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    monkeypatch.setattr(random, "random", lambda: 0.75)              # the area branch, as captured

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"torch.nn.functional.{name} was called on the HIP route")
        return f
    for name in ("conv1d", "layer_norm", "scaled_dot_product_attention", "batch_norm"):
        monkeypatch.setattr(F, name, refuse(name))



def test_module_train_mode_by_the_twin_criterion(hip_only):
    import dinodisc_spec as S
    tw = _small_twin()
    g = tw["g"]
    disc, _, _ = S.build_module(DEV)
    disc.train()
    with torch.autocast("cuda", dtype=BF):
        logits = disc(tw["x"].to(DEV))
    assert logits.shape == (12, 648) and logits.dtype == torch.float32
    _criterion("train logits", logits.detach().cpu(), tw["logits_train"], g.t("logits_train"))
    (logits * tw["dy"].to(DEV)).sum().backward()
    for k, p in disc.named_parameters():
        gr = p.grad.cpu()
        if k.endswith(".0.bias"):
            bound = ZERO_GRAD_FACTOR * float(g["gn." + k[:-4] + "weight_orig"])
            print(f"[fig] {k}: max |grad| {gr.abs().max().item():.3e} (twin {tw['grads'][k].abs().max().item():.3e}, bound {bound:.3e})")
            assert gr.abs().max().item() <= bound, k
            continue
        ref = g.t("g." + k) if "g." + k in g else g.t("gs." + k)
        _criterion("grad " + k, _sliced(k, gr), _sliced(k, tw["grads"][k]), ref)
    sd = disc.state_dict()
    for k in sd:
        if k.endswith(("weight_u", "weight_v")):
            assert rel_err(sd[k].cpu(), g.t("uv." + k)) < 2e-5, k          # f32 spectral norm: the CPU test's bar


def test_module_eval_mode_input_gradient_by_the_twin_criterion(hip_only):
    import dinodisc_spec as S
    tw = _small_twin()
    g = tw["g"]
    disc, _, heads = S.build_module(DEV)
    disc.eval().requires_grad_(False)
    x = tw["x"].to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        logits = disc(x)
    _criterion("eval logits", logits.detach().cpu(), tw["logits_eval"], g.t("logits_eval"))
    (logits * tw["dy"].to(DEV)).sum().backward()
    _criterion("dx", x.grad[:, :, ::16, ::16].cpu(), tw["dx"][:, :, ::16, ::16], g.t("dx_slice"))
    n_hip, n_twin, n_ref = x.grad.double().norm().item(), tw["dx"].double().norm().item(), float(g["dx_norm"])
    print(f"[fig] |dx|: HIP {n_hip:.4e}, twin {n_twin:.4e}, capture {n_ref:.4e}")      # a figure only: the slice's rel-L2 above is the check
    sd = disc.state_dict()
    assert all(torch.equal(sd[k].cpu(), heads[k]) for k in sd if k.endswith(("weight_u", "weight_v")))
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):             # the graph-free backbone route gives the bits of the route with the input gradient
        assert torch.equal(disc(tw["x"].to(DEV)), logits.detach())


def test_module_preprocessing_branches_by_the_twin_criterion(hip_only, monkeypatch):
    import dinodisc_spec as S
    from conftest import load_golden
    from oracle import ref_cpu as R
    from test_dinodisc_cpu import branch_inputs
    monkeypatch.undo()                                                   # the crop case draws from `random` itself ...
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)              # ... the stock route stays shut
    g, c = load_golden("dinodisc_branches"), S.SMALL
    disc, backbone, heads = S.build_module(DEV)
    disc.eval()
    for name, x, seed in branch_inputs(g):
        seed()
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            out = disc(x.to(DEV))
        crop = None
        if name == "crop":                                               # the offsets the module drew: the same generators, the same order
            seed()
            assert random.random() <= 0.5
            crop = (int(torch.randint(0, 256 - 252 + 1, size=(1,)).item()), int(torch.randint(0, 256 - 252 + 1, size=(1,)).item()))
        with torch.no_grad():
            twin = S.forward(x, backbone, heads, c["ks"], c["key_depths"], train=False, branch="crop" if crop else "bicubic", crop=crop, q=R.bf16_round)
        _criterion("branch " + name, out.cpu(), twin, g.t(name))


def test_trainer_steps_with_dinodisc_are_finite_and_repeat():
    """Two fresh TokenizerTrainer(disc=DinoDisc(reduced backbone), disc_start_step=0) on the step_small_w256 model, two steps each: finite logs, the same bits."""
    import dinodisc_spec as S
    from conftest import load_golden
    from test_oracle_golden import lpips_params
    from test_oracle_step import step_small_inputs
    from dmvae_amd.train import TokenizerTrainer
    from dmvae_amd.utils.lpips import LPIPS
    g = load_golden("step_small_w256")

    def run():
        p, vae, _, images = step_small_inputs(g)
        vae.load_state_dict(p, strict=True)
        lp = LPIPS().eval().requires_grad_(False)
        lp.load_state_dict(lpips_params(g, "lp."), strict=False)
        disc, _, _ = S.build_module(DEV, depth=2, key_depths=(0, 1))
        tr = TokenizerTrainer(vae.cuda(), lp.cuda(), lr=1e-4, warmup_steps=1, disc=disc, disc_start_step=0)
        random.seed(3)
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)
        out = [tr.step(images.cuda()).item() for _ in range(2)]
        return tr, out

    tr, out = run()
    log, dlog = tr.read_log(), tr.read_disc_log()
    assert all(v == v and abs(v) < 1e6 for v in list(log.values()) + list(dlog.values()) + out), (log, dlog, out)
    assert log["d_weight"] > 0 and dlog["disc_norm"] > 0
    tr2, out2 = run()
    assert out == out2 and torch.equal(tr.fp.flat, tr2.fp.flat) and torch.equal(tr.dfp.flat, tr2.dfp.flat)
    assert all(torch.equal(a, b) for a, b in zip(tr.disc.state_dict().values(), tr2.disc.state_dict().values()))


def test_module_with_groupnorm_heads(hip_only, monkeypatch):
    """norm_type='gn' (models/dinodisc.py:66-67: GroupNorm(32)) on the HIP route -- the GroupNorm kernels with n = B images and 32 groups of 12 channels -- against
    the module's own plain-PyTorch statement in f32 on the CPU.  No capture and no twin exist for this variant (no script passes it): the bar is 2e-2 rel-L2,
    twice what the bf16-site twin of the 'bn' module of the same depth measures against its capture (9.7e-3), for logits and for the input gradient's slice
    (twin: 7.4e-2 -> 1.5e-1); a wrong group geometry or a dropped affine moves both by far more."""
    import dinodisc_spec as S
    disc, _, _ = S.build_module(norm_type="gn")
    disc.eval().requires_grad_(False)
    x = S.image(4, 70, 2)
    dy = torch.randn(4, 50, generator=torch.Generator().manual_seed(1))
    monkeypatch.undo()                                                   # the CPU reference calls the stock functionals
    xc = x.clone().requires_grad_(True)
    want = disc.forward_stock(xc)
    (want * dy).sum().backward()
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    disc = disc.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        got = disc(xg)
    (got * dy.to(DEV)).sum().backward()
    e_y, e_dx = _rel_l2(got.detach().cpu(), want.detach()), _rel_l2(xg.grad.cpu(), xc.grad)
    print(f"[fig] gn heads: rel-L2 to the f32 CPU module -- logits {e_y:.3e}, dx {e_dx:.3e}")
    assert e_y < 2e-2 and e_dx < 1.5e-1
