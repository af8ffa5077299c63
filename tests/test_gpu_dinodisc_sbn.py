"""DinoDisc with SyncBatchNorm heads -- the configuration the reference's trainers build (norm_type "sbn", use_specnorm False; train_tokenizer.py:48-49,307-314) --
on an MI355X (-m gpu): the two kernels of the eval-mode head (the convolution's BatchNorm + LeakyReLU epilogue, its elementwise backward), the train-mode norm stage
with external statistics as the head runs it, the module in both modes with the stock functionals shut, a trainer, and two ranks.

Bars (none is taken from what the kernels give):
  epilogue, bnact_bwd   test_gpu_modules._assert_bf16_of against float64 on the kernel's OWN operands (<= 1 bf16 spacing, != RNE(f64) for <= 0.2 %), as the plain
                        token conv in tests/test_gpu_dinodisc.py; the f64 side uses the bf16 weight pack, the f32 vectors and the f32 values of eps and the slope
  train-mode norm       tests/test_gpu_dinodisc.py::test_batchnorm_local_leaky's: statistics 1e-5 relative (the mean: of |mean| + std of its channel), bf16 outputs
                        |err| <= 2^-8 |ref| + 1e-5 max |ref|, dgamma / dbeta rel_err 1e-5; dy zeroed where the f64 pre-activation has |u| < 1e-3, whose share
                        the f64 statement alone must keep under 5e-3; running_mean 1e-5 of (|mean| + std), running_var 1e-5 relative.  These bars are those of a
                        kernel on its own operands, so they are held where the head's norm runs -- `functional._dino_norm_fwd` / `_dino_norm_bwd`, the two
                        functions `DinoHeadFn` calls -- with the tail checked on the Function's own stored a, h (rel_err 1e-5, test_head_tail's bar); the Function
                        end to end is held by the module tests below
  module                the bf16-site criterion of tests/test_gpu_dinodisc.py (`_criterion`): rel-L2 to the reference's f32 capture no more than 1.15 x that of
                        the CPU twin with bf16 rounding at the HIP route's storage sites (tests/dinodisc_sbn_spec.py); conv biases in front of a train-mode norm
                        (analytically zero gradient) bounded by 2^-8 of the same conv's weight-gradient norm, as there

Figures observed on an MI355X (module tests; rel-L2 to the reference's f32 capture, HIP route / CPU twin):
  train logits 9.42e-3 / 9.39e-3, second call 9.13e-3 / 9.35e-3; the 14 head gradients no bf16 site leaves alone: ratio HIP / twin 0.93 ... 1.10 (errors 6.3e-3 ...
  8.1e-2); the last biases' gradients 4.8e-7 and 6.6e-8 [1e-5]; zero-gradient conv biases max |grad| 1.9e-2 ... 6.6e-2 [bounds 3.4 ... 7.2]; running statistics after
  the first and second call: ratio 0.92 ... 1.03 (errors 2.3e-5 ... 3.7e-3); eval logits 6.60e-3 / 6.81e-3, dx 5.39e-2 / 5.62e-2; composed 6.95e-3 / 7.14e-3,
  5.47e-2 / 5.64e-2.  The two-rank test needs two GPUs and has not run on a device yet.
"""
import functools
import random
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from test_gpu_dinodisc import CONV_CASES, F32_LEVEL, SLOPE, ZERO_GRAD_FACTOR, _conv_case, _criterion, _ops, _packs, _sliced

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
EPS = float(np.float32(1e-6))
STATE = ("running_mean", "running_var", "num_batches_tracked")


@pytest.fixture
def syncbn_on(monkeypatch):
    import dmvae_amd.models.dinodisc as D
    monkeypatch.setattr(D, "_SYNCBN_HEADS", True)


# ---- the eval-mode head's two kernels --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bn_vectors(c):
    """running_mean, running_var, gamma, beta [C] f32; gamma negative in channels 0..3, zero in 4..7, large in 8..11."""
    g = torch.Generator().manual_seed(c)
    rm, rv = 0.3 * torch.randn(c, generator=g), torch.rand(c, generator=g) * 1.5 + 0.1
    gamma, beta = 1 + 0.5 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    gamma[0:4] = -gamma[0:4].abs() - 0.1
    gamma[4:8] = 0.0
    gamma[8:12] = 50.0
    return rm, rv, gamma, beta


def _bnact64(y64, c):
    rm, rv, gamma, beta = (v.double() for v in _bn_vectors(c))
    u = (y64 - rm) / torch.sqrt(rv + EPS) * gamma + beta
    return torch.where(u > 0, u, SLOPE * u)


@pytest.mark.parametrize("b,l,c,ks", CONV_CASES)
def test_conv_tokens_bnact_epilogue(b, l, c, ks):
    from test_gpu_modules import _assert_bf16_of
    ops = _ops()
    case = _conv_case(b, l, c, ks)
    wf, _ = _packs(case)
    x, bias = case["x"].to(DEV), case["bias"].to(DEV)
    bn = tuple(v.to(DEV) for v in _bn_vectors(c)) + (EPS,)
    y = ops.conv_tokens(x, wf, bias, bn=bn)
    _assert_bf16_of(y, _bnact64(case["y"], c), f"conv_tokens + bnact {b, l, c, ks}")
    assert (y[..., 4:8].float().cpu() == F.leaky_relu(_bn_vectors(c)[3][4:8], SLOPE).to(BF).float()).all()       # gamma = 0: leaky(beta), whatever the conv gives
    assert torch.equal(y, ops.conv_tokens(x, wf, bias, bn=bn))
    for i in range(b):                                                     # a sample's result does not depend on the batch it is in
        assert torch.equal(y[i:i + 1], ops.conv_tokens(x[i:i + 1].contiguous(), wf, bias, bn=bn))
    y0 = ops.conv_tokens(x, wf, None, bn=bn)                               # no bias
    _assert_bf16_of(y0, _bnact64(case["y"] - case["bias"].double(), c), f"conv_tokens + bnact without bias {b, l, c, ks}")
    plain = ops.conv_tokens(x, wf, bias)                                   # the plain entry point beside it: still the rounding of its f64 value, still itself
    _assert_bf16_of(plain, case["y"], f"conv_tokens {b, l, c, ks}")
    assert torch.equal(plain, ops.conv_tokens(x, wf, bias)) and not torch.equal(plain, y)


@pytest.mark.parametrize("b,l,c,ks", CONV_CASES)
def test_dino_bnact_bwd(b, l, c, ks):
    from test_gpu_modules import _assert_bf16_of
    ops = _ops()
    case = _conv_case(b, l, c, ks)
    wf, _ = _packs(case)
    _, rv, gamma, _ = _bn_vectors(c)
    bn = tuple(v.to(DEV) for v in _bn_vectors(c)) + (EPS,)
    y = ops.conv_tokens(case["x"].to(DEV), wf, case["bias"].to(DEV), bn=bn).clone()      # the mask comes from the kernel's own stored output
    y[:, 0, 16:24] = 0.0                                                    # exact zeros of both signs: the slope, as ATen's backward at 0
    y[:, -1, 24:32] = -0.0
    dy = case["dy"].to(DEV)
    g = ops.dino_bnact_bwd(dy, y, bn[2], bn[1], EPS)
    yc = y.float().cpu()
    assert (yc[:, 0, 16:24] == 0).all() and torch.signbit(yc[:, -1, 24:32]).all() and (yc > 0).any() and (yc < 0).any()
    ref = case["dy"].double() * torch.where(yc > 0, 1.0, SLOPE).double() * gamma.double() / torch.sqrt(rv.double() + EPS)
    _assert_bf16_of(g, ref, f"dino_bnact_bwd {b, l, c}")
    assert (g[..., 4:8] == 0).all()                                         # gamma = 0
    assert torch.equal(g, ops.dino_bnact_bwd(dy, y, bn[2], bn[1], EPS))


def test_bnact_entry_points_refuse_what_they_do_not_cover():
    from dmvae_amd._lib import DmvaeHipError
    ops = _ops()
    v = torch.ones(256, device=DEV)
    with pytest.raises(DmvaeHipError, match="multiple of 32 in 384"):
        ops.conv_tokens(torch.zeros(1, 4, 256, dtype=BF, device=DEV), torch.zeros(256, 3, 256, dtype=BF, device=DEV), None, bn=(v, v, v, v, EPS))
    z = torch.zeros(1, 4, 12, dtype=BF, device=DEV)
    with pytest.raises(DmvaeHipError, match="multiple of 8"):
        ops.dino_bnact_bwd(z, z, v[:12].contiguous(), v[:12].contiguous(), EPS)


# ---- the train-mode norm stage with external statistics --------------------------------------------------------------------------------------------------------
NORM_CASES = [(12, 25), (2, 324)]             # the 70 px grid at the captures' batch; the production grid (test_batchnorm_local_leaky's second shape)


@functools.lru_cache(maxsize=None)
def _norm_case(b, l, c=384):
    """SyncBatchNorm + LeakyReLU on token-major [B, L, C] in float64 on bf16 operands: one "image" of B * L rows, one channel per group; dy zeroed where the
    pre-activation is within 1e-3 of the kink.  Computed once per shape, never written to."""
    g = torch.Generator().manual_seed(100 * b + l)
    mu, sd = torch.rand(c, generator=g) * 6 - 3, torch.rand(c, generator=g) * 1.8 + 0.2
    x = (torch.randn(b, l, c, generator=g) * sd + mu).to(BF)
    gamma, beta = 1 + 0.5 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    da = torch.randn(b, l, c, generator=g).to(BF)
    rm0, rv0 = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    x64 = x.double().view(1, b * l, c).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mean, var = x64.mean(1, keepdim=True), x64.var(1, unbiased=False, keepdim=True)
    u = (x64 - mean) / torch.sqrt(var + EPS) * g64 + b64
    amb = u.detach().abs() < 1e-3
    share = amb.double().mean().item()
    da_used = da.view(1, b * l, c).masked_fill(amb, 0)
    y = F.leaky_relu(u, SLOPE)
    y.backward(da_used.double())
    n = b * l
    return dict(x=x, gamma=gamma, beta=beta, da=da_used.view(b, l, c).contiguous(), rm0=rm0, rv0=rv0, share=share, mean=mean.detach()[0, 0], var=var.detach()[0, 0],
                y=y.detach().view(b, l, c), dx=x64.grad.view(b, l, c), dg=g64.grad, db=b64.grad,
                rm1=0.9 * rm0.double() + 0.1 * mean.detach()[0, 0], rv1=0.9 * rv0.double() + 0.1 * var.detach()[0, 0] * n / (n - 1))


def _bf16_bar(got, ref):
    return ((got.double().cpu() - ref).abs() / (2.0 ** -8 * ref.abs() + 1e-5 * ref.abs().max())).max().item()


def _check_norm_stage(case, lo, hi, bn, y, st, dx, dg, db, sum_param_grads=None):
    """Samples lo:hi of the case (all of it on one rank) against the float64 statement of the whole batch."""
    scale = case["mean"].abs() + case["var"].sqrt()
    assert ((st[0, :, 0].cpu().double() - case["mean"]).abs() <= 1e-5 * scale).all()
    rstd = 1 / torch.sqrt(case["var"] + EPS)
    assert ((st[0, :, 1].cpu().double() - rstd).abs() <= 1e-5 * rstd).all()
    assert _bf16_bar(y, case["y"][lo:hi]) <= 1.0
    assert _bf16_bar(dx, case["dx"][lo:hi]) <= 1.0
    if sum_param_grads is not None:
        sum_param_grads(dg, db)
    assert rel_err(dg.cpu(), case["dg"]) < 1e-5 and rel_err(db.cpu(), case["db"]) < 1e-5
    assert ((bn.running_mean.cpu().double() - case["rm1"]).abs() <= 1e-5 * scale).all()
    assert ((bn.running_var.cpu().double() - case["rv1"]).abs() <= 1e-5 * case["rv1"]).all()
    assert int(bn.num_batches_tracked) == 1


def _sync_bn(case, c=384):
    bn = torch.nn.SyncBatchNorm(c, eps=EPS).to(DEV).train()
    with torch.no_grad():
        bn.running_mean.copy_(case["rm0"])
        bn.running_var.copy_(case["rv0"])
    return bn


@pytest.mark.parametrize("b,l", NORM_CASES)
def test_train_mode_norm_stage_with_external_statistics(b, l):
    """nimg = 1, groups = C, the statistics through models.patchgan._bn_stats bound to an nn.SyncBatchNorm (a single rank: its one-launch running update), the
    backward split into reduce and apply with 1 / count: the two functions DinoHeadFn calls, on their own operands."""
    from dmvae_amd.functional import _dino_norm_bwd, _dino_norm_fwd
    from dmvae_amd.models.patchgan import _bn_stats
    case = _norm_case(b, l)
    assert case["share"] < 5e-3                                            # the float64 statement alone keeps the ambiguous share under the cap
    c = 384
    bn = _sync_bn(case)
    x, gamma, beta, da = (case[k].to(DEV) for k in ("x", "gamma", "beta", "da"))
    y, st, sync = _dino_norm_fwd(x, gamma, beta, 1, c, EPS, partial(_bn_stats, bn))
    assert sync == [True, b * l, None]
    dx, dg, db = _dino_norm_bwd(da, x, st, gamma, beta, 1, c, True, sync)
    _check_norm_stage(case, 0, b, bn, y, st, dx.view(b, l, c), dg, db)
    dx2, none_g, none_b = _dino_norm_bwd(da, x, st, gamma, beta, 1, c, False, sync)       # frozen heads
    assert none_g is None and none_b is None and torch.equal(dx2, dx)
    # eval mode with heads that train (the composed route): the running estimates as constants, no update, zero sums
    bn.eval()
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    ye, ste, synce = _dino_norm_fwd(x, gamma, beta, 1, c, EPS, partial(_bn_stats, bn))
    assert synce[0] is False and torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv) and int(bn.num_batches_tracked) == 1
    x64 = case["x"].double().requires_grad_(True)
    g64 = case["gamma"].double().requires_grad_(True)
    u = (x64 - rm.cpu().double()) / torch.sqrt(rv.cpu().double() + EPS) * g64 + case["beta"].double()
    amb = u.detach().abs() < 1e-3
    assert amb.double().mean().item() < 5e-3
    dae = case["da"].masked_fill(amb, 0)
    F.leaky_relu(u, SLOPE).backward(dae.double())
    dxe, dge, _ = _dino_norm_bwd(dae.to(DEV), x, ste, gamma, beta, 1, c, True, synce)
    assert _bf16_bar(ye, F.leaky_relu(u.detach(), SLOPE)) <= 1.0 and _bf16_bar(dxe.view(b, l, c), x64.grad) <= 1.0 and rel_err(dge.cpu(), g64.grad) < 1e-5


def test_head_function_with_external_statistics_runs_the_norm_stage(syncbn_on):
    """DinoHeadFn with cfg (1, C, eps, statistics callables): its stored tensors are those of the norm stage above on its own conv results, its logits the tail of
    its stored a, h (rel_err 1e-5), the running estimates move once per norm and call, and every gradient it is asked for comes back finite and repeatable."""
    from dmvae_amd.functional import DinoHeadFn, _dino_norm_fwd
    from dmvae_amd.models.patchgan import _bn_stats
    ops = _ops()
    b, l, c, ks = 3, 25, 384, 9
    g = torch.Generator().manual_seed(9)
    t = (torch.randn(b, l + 1, c, generator=g) * 2).to(DEV).requires_grad_(True)
    mk = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(DEV).requires_grad_(True)
    w0, b0, w1, b1, w2, b2 = mk(c, c, 1, k=c ** -0.5), mk(c, k=0.1), mk(c, c, ks, k=(c * ks) ** -0.5), mk(c, k=0.1), mk(1, c, 1, k=c ** -0.5), mk(1, k=0.1)
    g0, be0, g1, be1 = (1 + mk(c, k=0.3)).detach().requires_grad_(True), mk(c, k=0.3), (1 + mk(c, k=0.3)).detach().requires_grad_(True), mk(c, k=0.3)
    one = torch.ones(1, device=DEV)

    def run():
        n0, n1 = (torch.nn.SyncBatchNorm(c, eps=EPS).to(DEV).train() for _ in range(2))
        logit = DinoHeadFn.apply(t, (1, c, EPS, (partial(_bn_stats, n0), partial(_bn_stats, n1))), w0, one, b0, g0, be0, w1, one, b1, g1, be1, w2, one, b2)
        dl = torch.randn(b, l, generator=torch.Generator().manual_seed(1)).to(DEV)
        grads = torch.autograd.grad(logit, [t, w0, b0, g0, be0, w1, b1, g1, be1, w2, b2], dl, retain_graph=True)
        return logit, grads, n0, n1

    logit, grads, n0, n1 = run()
    act, h0, st0, a, c1, st1, h = logit.grad_fn.saved_tensors[:7]
    assert int(n0.num_batches_tracked) == 1 and int(n1.num_batches_tracked) == 1
    for x_, st_, g_, be_, y_, n_ in ((h0, st0, g0, be0, a, n0), (c1, st1, g1, be1, h, n1)):
        fresh = torch.nn.SyncBatchNorm(c, eps=EPS).to(DEV).train()
        y2, st2, _ = _dino_norm_fwd(x_, g_.detach(), be_.detach(), 1, c, EPS, partial(_bn_stats, fresh))
        assert torch.equal(y2, y_) and torch.equal(st2, st_) and torch.equal(fresh.running_mean, n_.running_mean) and torch.equal(fresh.running_var, n_.running_var)
    ref = ((a.double() + h.double()) / np.sqrt(2) * w2.detach().double().view(c)).sum(-1) + b2.detach().double()
    assert rel_err(logit.detach(), ref) < 1e-5
    logit2, grads2, _, _ = run()
    assert torch.equal(logit, logit2) and all(torch.isfinite(x_).all() and torch.equal(x_, y_) for x_, y_ in zip(grads, grads2))
    assert torch.equal(ops.dino_tap(t.detach()), act)


# ---- the module, stock functionals shut ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_twin():
    """The capture and the twin's results on it (CPU, bf16 sites), computed once."""
    import dinodisc_spec as S
    import dinodisc_sbn_spec as SB
    import dmvae_amd.models.dinodisc as D
    from conftest import load_golden
    from oracle import ref_cpu as R
    g, c = load_golden("dinodisc_sbn_small"), SB.SMALL
    was = D.enable_syncbn_heads()
    try:
        _, backbone, heads = SB.build_module()
    finally:
        D.enable_syncbn_heads(was)
    x, x2 = S.image(c["batch"], c["px"], c["x_seed"]), S.image(c["batch"], c["px"], c["x_seed"] + 1)
    dy = torch.randn(12, 648, generator=torch.Generator().manual_seed(c["dy_seed"]))
    p = {k: v.clone().requires_grad_(SB.is_param(k)) for k, v in heads.items()}
    st1, st2 = {}, {}
    lt = SB.forward(x, backbone, p, train=True, q=R.bf16_round, new_state=st1)
    (lt * dy).sum().backward()
    with torch.no_grad():
        lt2 = SB.forward(x2, backbone, {**heads, **st1}, train=True, q=R.bf16_round, new_state=st2)
    out = dict(g=g, x=x, x2=x2, dy=dy, logits_train=lt.detach(), logits_train2=lt2, st1=st1, st2=st2, grads={k: v.grad for k, v in p.items() if v.requires_grad})
    for name, fused in (("", True), ("_composed", False)):
        xe = x.clone().requires_grad_(True)
        le = SB.forward(xe, backbone, heads, train=False, q=R.bf16_round, fused_eval=fused)
        (le * dy).sum().backward()
        out["logits_eval" + name], out["dx" + name] = le.detach(), xe.grad
    return out


@pytest.fixture
def hip_only(monkeypatch, syncbn_on):
    """The route under test is the HIP route: no opt-in to the stock modules, and the stock functionals raise."""
    _small_twin()
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    monkeypatch.setattr(random, "random", lambda: 0.75)              # the area branch, as captured

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"torch.nn.functional.{name} was called on the HIP route")
        return f
    for name in ("conv1d", "layer_norm", "scaled_dot_product_attention", "batch_norm", "leaky_relu"):
        monkeypatch.setattr(F, name, refuse(name))


def _graph_has(fn, name, depth=4):
    """Whether an autograd node whose type name starts with `name` sits within `depth` edges of fn."""
    if fn is None or depth < 0:
        return False
    return type(fn).__name__.startswith(name) or any(_graph_has(nxt, name, depth - 1) for nxt, _ in fn.next_functions)


def _check_state(tw, tag, disc):
    g = tw["g"]
    sd = disc.state_dict()
    for k in sd:
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(g[tag + "." + k]) == int(tw[tag][k]), k
        elif k.endswith(STATE):
            _criterion(f"{tag} {k}", sd[k].cpu(), tw[tag][k], g.t(tag + "." + k))


def test_module_train_mode_by_the_twin_criterion(hip_only):
    import dinodisc_sbn_spec as SB
    tw = _small_twin()
    g = tw["g"]
    disc, _, _ = SB.build_module(DEV)
    disc.train()
    with torch.autocast("cuda", dtype=BF):
        logits = disc(tw["x"].to(DEV))
    assert logits.shape == (12, 648) and logits.dtype == torch.float32
    _criterion("train logits", logits.detach().cpu(), tw["logits_train"], g.t("logits_train"))
    (logits * tw["dy"].to(DEV)).sum().backward()
    for k, p in disc.named_parameters():
        gr = p.grad.cpu()
        if k.endswith(".0.bias"):
            bound = ZERO_GRAD_FACTOR * float(g["gn." + k[:-4] + "weight"])
            print(f"[fig] {k}: max |grad| {gr.abs().max().item():.3e} (twin {tw['grads'][k].abs().max().item():.3e}, bound {bound:.3e})")
            assert gr.abs().max().item() <= bound, k
            continue
        ref = g.t("g." + k) if "g." + k in g else g.t("gs." + k)
        _criterion("grad " + k, _sliced(k, gr), _sliced(k, tw["grads"][k]), ref)
    _check_state(tw, "st1", disc)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        logits2 = disc(tw["x2"].to(DEV))
    _criterion("train logits, second call", logits2.cpu(), tw["logits_train2"], g.t("logits_train2"))
    _check_state(tw, "st2", disc)


def test_module_eval_mode_input_gradient_by_the_twin_criterion(hip_only):
    import dinodisc_sbn_spec as SB
    tw = _small_twin()
    g = tw["g"]
    disc, _, heads = SB.build_module(DEV)
    disc.eval().requires_grad_(False)
    x = tw["x"].to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        logits = disc(x)
    assert _graph_has(logits.grad_fn, "DinoHeadEvalFn") and not _graph_has(logits.grad_fn, "DinoHeadFnBackward")
    _criterion("eval logits", logits.detach().cpu(), tw["logits_eval"], g.t("logits_eval"))
    (logits * tw["dy"].to(DEV)).sum().backward()
    _criterion("dx", x.grad[:, :, ::16, ::16].cpu(), tw["dx"][:, :, ::16, ::16], g.t("dx_slice"))
    sd = disc.state_dict()
    assert all(torch.equal(sd[k].cpu(), heads[k]) for k in sd if k.endswith(STATE))                    # eval: the estimates are constants
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):             # the graph-free backbone route gives the bits of the route with the input gradient
        assert torch.equal(disc(tw["x"].to(DEV)), logits.detach())
    # heads that train, in eval mode (not a case of the trainers): the composed route with constant statistics
    disc.requires_grad_(True)
    xc = tw["x"].to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        lc = disc(xc)
    _criterion("eval logits, composed", lc.detach().cpu(), tw["logits_eval_composed"], g.t("logits_eval"))
    (lc * tw["dy"].to(DEV)).sum().backward()
    _criterion("dx, composed", xc.grad[:, :, ::16, ::16].cpu(), tw["dx_composed"][:, :, ::16, ::16], g.t("dx_slice"))
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in disc.parameters())
    sd = disc.state_dict()
    assert all(torch.equal(sd[k].cpu(), heads[k]) for k in sd if k.endswith(STATE))


def test_trainer_steps_with_syncbn_dinodisc_are_finite_repeat_and_checkpoint(syncbn_on):
    """Two fresh TokenizerTrainer(disc=DinoDisc(sbn, no spectral norm, reduced backbone), disc_start_step=0) on the step_small_w256 model, two steps each: finite
    logs, the same bits; the counter moves twice per step (the discriminator's turn calls the module twice, train_tokenizer.py:212,217; the generator's term runs
    in eval mode), and checkpoint() / load carries the running statistics and the counter."""
    import dinodisc_sbn_spec as SB
    from conftest import load_golden
    from test_oracle_golden import lpips_params
    from test_oracle_step import step_small_inputs
    from dmvae_amd.train import TokenizerTrainer
    from dmvae_amd.utils.lpips import LPIPS
    g = load_golden("step_small_w256")

    def run(steps):
        p, vae, _, images = step_small_inputs(g)
        vae.load_state_dict(p, strict=True)
        lp = LPIPS().eval().requires_grad_(False)
        lp.load_state_dict(lpips_params(g, "lp."), strict=False)
        disc, _, _ = SB.build_module(DEV, depth=2, key_depths=(0, 1))
        tr = TokenizerTrainer(vae.cuda(), lp.cuda(), lr=1e-4, warmup_steps=1, disc=disc, disc_start_step=0)
        random.seed(3)
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)
        out = [tr.step(images.cuda()).item() for _ in range(steps)]
        return tr, out

    tr, out = run(2)
    log, dlog = tr.read_log(), tr.read_disc_log()
    assert all(v == v and abs(v) < 1e6 for v in list(log.values()) + list(dlog.values()) + out), (log, dlog, out)
    assert log["d_weight"] > 0 and dlog["disc_norm"] > 0
    tr2, out2 = run(2)
    assert out == out2 and torch.equal(tr.fp.flat, tr2.fp.flat) and torch.equal(tr.dfp.flat, tr2.dfp.flat)
    sd, sd2 = tr.disc.state_dict(), tr2.disc.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    tracked = [k for k in sd if k.endswith("num_batches_tracked")]
    assert len(tracked) == 4 and all(int(sd[k]) == SB.TRACKED0 + 4 for k in tracked)
    ck = tr.checkpoint()
    stats = [k for k in ck["disc_wo_ddp"] if k.endswith(STATE)]
    assert len(stats) == 12
    with torch.no_grad():
        for k, v in tr2.disc.state_dict().items():
            if k.endswith(STATE):
                v.zero_()
    tr2.load(ck)
    sd2 = tr2.disc.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd) and int(sd2[tracked[0]]) == SB.TRACKED0 + 4


# ---- two ranks ---------------------------------------------------------------------------------------------------------------------------------------------------
def _two_gpu_worker(rank, port, q):
    import os
    os.environ.update(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as tdist
    from dmvae_amd import dist
    from dmvae_amd.functional import _dino_norm_bwd, _dino_norm_fwd
    from dmvae_amd.models.patchgan import _bn_stats
    dist.init_distributed_mode(backend="nccl")
    b, l, c = 12, 25, 384
    case = _norm_case(b, l)
    lo, hi = 6 * rank, 6 * rank + 6
    bn = _sync_bn(case)
    x, da = case["x"][lo:hi].contiguous().to(DEV), case["da"][lo:hi].contiguous().to(DEV)
    gamma, beta = case["gamma"].to(DEV), case["beta"].to(DEV)
    y, st, sync = _dino_norm_fwd(x, gamma, beta, 1, c, EPS, partial(_bn_stats, bn))
    ok = sync[0] is True and sync[1] == b * l and sync[2] is not None
    dx, dg, db = _dino_norm_bwd(da, x, st, gamma, beta, 1, c, True, sync)

    def sum_param_grads(dg, db):            # a rank's parameter gradients are its share: DDP / the flat-gradient all-reduce sums them
        tdist.all_reduce(dg)
        tdist.all_reduce(db)
    try:
        _check_norm_stage(case, lo, hi, bn, y, st, dx.view(6, l, c), dg, db, sum_param_grads)
    except AssertionError as e:
        ok = False
        print(f"rank {rank}: {e!r}", flush=True)
    dist.barrier()
    q.put((rank, bool(ok)))
    tdist.destroy_process_group()


def test_two_ranks_against_the_union_batch():
    """Two ranks of 6 samples each, over NCCL: each rank's statistics, output, input gradient, (summed) parameter gradients and running estimates against the
    float64 statement of the union batch of 12, by the bars of the single-rank test -- each side against float64, not against the other."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    import torch.multiprocessing as mp
    from test_dist_gloo import _free_port
    assert _norm_case(12, 25)["share"] < 5e-3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_gpu_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    assert sorted(q.get(timeout=5) for _ in range(2)) == [(0, True), (1, True)]
