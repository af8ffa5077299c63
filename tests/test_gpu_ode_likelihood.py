"""The likelihood sampler on the MI355X (-m gpu): `Sampler.sample_ode_likelihood()` (the reference's transport.py:402-459) on a CUDA f32 (x, logp) state.
The Hutchinson pack kernel (csrc/sampler.hip) against its float64 definition; the whole tuple-state dopri5 against its composed route, the float64 tuple
spec (tests/dopri5_tuple_spec.py) and the closed-form likelihood of Gaussian data; the per-evaluation trace estimate against a dense Jacobian; the frozen
LightningDiT's input-gradient route (csrc/dit_stack.hip / dit.hip dx-only kernels) against the training route and the reference's capture; and DiT-XL/1
through the public interface."""
import copy

import numpy as np
import pytest
import torch

import dopri5_tuple_spec as TS
from conftest import load_golden
from oracle import ref_cpu as R
from test_oracle_dit import CFGS, build
from test_oracle_ode_likelihood import ATOL, RTOL, _grid

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _rl2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


# ---- the pack kernel ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", [torch.float32, BF])
@pytest.mark.parametrize("shape", [(2, 7), (17, 241), (25, 32, 16, 16), (3, 5, 3, 3), (1, 4097)])
def test_hutchinson_pack_vs_f64(shape, vdtype):
    from dmvae_amd import ops
    g = torch.Generator(device=DEV).manual_seed(sum(shape))
    v = (torch.randn(shape, device=DEV, generator=g) * 3).to(vdtype)
    grad = torch.randn(shape, device=DEV, generator=g) * 10
    eps = torch.randint(2, shape, dtype=torch.float, device=DEV, generator=g) * 2 - 1
    out = ops.ode_hutchinson_pack(v, grad, eps)
    b, nx = shape[0], v.numel()
    assert out.shape == (nx + b,) and out.dtype == torch.float32
    assert torch.equal(out[:nx], -v.float().reshape(-1))                           # exact
    want = (grad.double() * eps.double()).reshape(b, -1).sum(1)
    assert torch.equal(out[nx:], want.float()) or (out[nx:].double() - want).abs().max() <= 2 ** -23 * want.abs().max() * 2
    again = torch.full_like(out, float("nan"))
    ops.ode_hutchinson_pack(v, grad, eps, out=again)
    assert torch.equal(out, again)


def test_hutchinson_pack_validates_inputs():
    from dmvae_amd import ops
    v = torch.randn(4, 8, device=DEV)
    e = torch.ones(4, 8, device=DEV)
    with pytest.raises(TypeError):
        ops.ode_hutchinson_pack(v, e.double(), e)
    with pytest.raises(ValueError):
        ops.ode_hutchinson_pack(v, torch.ones(8, 4, device=DEV).t(), e)
    with pytest.raises(ValueError):
        ops.ode_hutchinson_pack(v, torch.ones(4, 9, device=DEV), e)
    with pytest.raises(ValueError):
        ops.ode_hutchinson_pack(v, e, e, out=torch.empty(33, device=DEV))


# ---- the whole integrator on Gaussian data ---------------------------------------------------------------------------------------------------------------
S_DATA, D_SHAPE, B = 0.6, (3, 8, 8), 4


def _gaussian_model(x, t):
    """The exact velocity of N(0, s^2 I) data on the Linear path, from torch ops: v = x a(t)."""
    tt = t.double().view(-1, *([1] * (x.dim() - 1)))
    return (x.double() * TS.gaussian_rate(tt, S_DATA)).float()


def _likelihood(fused, model, x, seed=0, **kw):
    import dmvae_amd.transport as T
    from dmvae_amd.transport import Sampler, create_transport
    T.FUSED_STATE_UPDATE = fused
    try:
        fn = Sampler(create_transport()).sample_ode_likelihood(**kw)
        torch.manual_seed(seed)
        logp, z = fn(x, model)
        o = fn.ode
        return logp, z, (o.nfe, o.n_accepted, o.n_rejected)
    finally:
        T.FUSED_STATE_UPDATE = True


def test_integrator_gaussian_fused_composed_spec_and_closed_form():
    x = torch.randn(B, *D_SHAPE, generator=torch.Generator().manual_seed(2)).to(DEV) * S_DATA
    lf, zf, cf = _likelihood(True, _gaussian_model, x)
    lc, zc, cc = _likelihood(False, _gaussian_model, x)
    assert cf == cc and cf[0] == 2 + 6 * (cf[1] + cf[2])
    assert lf.shape == (B,) and zf.shape == x.shape and torch.isfinite(lf).all()
    assert (lf - lc).abs().max().item() < 1e-5 * lc.abs().max().item() and (zf - zc).abs().max().item() < 1e-5
    # the float64 tuple spec: the same steps, logp within f32 rounding
    d = int(np.prod(D_SHAPE))
    xn = x.double().cpu().numpy().reshape(B, d)
    y0 = np.concatenate([xn.ravel(), np.zeros(B)])
    parts = [(0, B * d), (B * d, B * d + B)]
    out, steps, nfe = TS.solve(TS.gaussian_likelihood_drift(S_DATA, d, B), y0, _grid(), ATOL, RTOL, parts=parts)
    assert min(abs(st[2] - 1) for st in steps) > 1e-3
    assert cf == (nfe, sum(st[3] for st in steps), sum(not st[3] for st in steps))
    z_spec, dl_spec = out[-1][:B * d].reshape(B, d), out[-1][B * d:]
    logp_spec = (-d / 2 * np.log(2 * np.pi) - (z_spec ** 2).sum(1) / 2) - dl_spec
    assert np.abs(lf.double().cpu().numpy() - logp_spec).max() < 1e-4 * np.abs(logp_spec).max()         # f32 state over ~100 steps
    # the closed form, within the spec's own distance to it at atol 1e-6 / rtol 1e-3
    want, want_z = TS.gaussian_logp(xn, S_DATA)
    spec_err = np.abs(logp_spec - want).max()
    assert np.abs(lf.double().cpu().numpy() - want).max() < 2 * spec_err + 1e-4 * np.abs(want).max()
    zg = zf.double().cpu().numpy().reshape(B, d)
    assert np.abs(zg - z_spec).max() < 1e-4 * np.abs(z_spec).max()              # the f32 state, as logp above
    assert np.abs(zg - want_z).max() < 2 * np.abs(z_spec - want_z).max() + 1e-4 * np.abs(want_z).max()


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_fixed_grid_methods_take_the_tuple_state(method):
    x = torch.randn(B, *D_SHAPE, generator=torch.Generator().manual_seed(4)).to(DEV) * S_DATA
    lf, zf, _ = _likelihood(True, _gaussian_model, x, sampling_method=method, num_steps=200)
    lc, zc, _ = _likelihood(False, _gaussian_model, x, sampling_method=method, num_steps=200)
    want, _ = TS.gaussian_logp(x.double().cpu().numpy().reshape(B, -1), S_DATA)
    assert (lf - lc).abs().max().item() < 1e-4 * lc.abs().max().item()
    tol = 0.05 if method == "euler" else 1e-4
    assert np.abs(lf.double().cpu().numpy() - want).max() < tol * np.abs(want).max()


def test_per_evaluation_trace_estimate_is_eps_J_eps():
    """logp_grad == eps^T J eps (J the dense float64 Jacobian of a small non-diagonal nonlinear model), for the drift's tensor form and its packed kernel
    form alike; -v is the model output exactly."""
    from dmvae_amd.transport import Sampler, create_transport
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(12, 12, generator=g, dtype=torch.float64) * 0.4).to(DEV)

    def model(x, t):
        f = x.reshape(x.shape[0], -1)
        return (torch.tanh(f @ w.to(f.dtype)) * f.roll(1, 1) + t.view(-1, 1) * f ** 2).view_as(x)

    drift = Sampler(create_transport()).sample_ode_likelihood().ode.drift
    x = torch.randn(5, 3, 2, 2, generator=g).to(DEV)
    t = torch.full((5,), 0.25, device=DEV)
    torch.manual_seed(3)
    neg_v, lg = drift((x, torch.zeros(5, device=DEV)), t, model)
    out = torch.empty(x.numel() + 5, device=DEV)
    torch.manual_seed(3)
    drift.packed((x, torch.zeros(5, device=DEV)), t, model, out=out)
    torch.manual_seed(3)
    eps = torch.randint(2, x.size(), dtype=torch.float, device=DEV) * 2 - 1
    assert torch.equal(neg_v, -model(x, torch.full((5,), 0.75, device=DEV)))
    assert torch.equal(out[:x.numel()], neg_v.reshape(-1))
    for i in range(5):
        f = lambda r: model(r.view(1, 3, 2, 2), torch.full((1,), 0.75, dtype=torch.float64, device=DEV)).reshape(-1)
        jac = torch.autograd.functional.jacobian(f, x[i].double())
        jm = jac.reshape(12, 12)
        assert (jm - torch.diag(jm.diagonal())).abs().max() > 0.05                                  # not diagonal
        e = eps[i].reshape(-1).double()
        want = (e @ jac.reshape(12, 12) @ e).item()
        assert abs(lg[i].item() - want) < 1e-5 * max(1.0, abs(want)), (i, lg[i].item(), want)
        assert abs(out[x.numel() + i].item() - want) < 1e-5 * max(1.0, abs(want))


# ---- the frozen DiT's input-gradient route ---------------------------------------------------------------------------------------------------------------
def _frozen_copy(m):
    f = copy.deepcopy(m)
    f.requires_grad_(False)
    return f


def _forbid_weight_gradients(monkeypatch):
    from dmvae_amd import ops

    def boom(*a, **k):
        raise AssertionError("a weight-gradient entry point was called on the input-gradient route")
    for name in ("linear_wgrad_grouped", "linear_rows_wgrad_batched", "linear_rows_wgrad", "conv2d_nhwc_wgrad", "rmsnorm_modulate_bwd_"):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(ops.DitStackBwd, "finalize", boom)


@pytest.mark.parametrize("tag", ["dit_small_hd64w", "dit_small_hd72"])
def test_dit_input_vjp_frozen(tag, monkeypatch):
    from dmvae_amd import functional as Fn
    from dmvae_amd.models import lightningdit_fast as LF
    g = load_golden(tag)
    m = build(tag, g).to(DEV)
    fz = _frozen_copy(m)
    x, t, y = g.t("x").to(DEV), g.t("t").to(DEV), torch.from_numpy(np.asarray(g["y"])).to(DEV)
    dy = g.t("dy").to(DEV)
    stack = Fn.dit_stack_supported(x.shape[0], m.x_embedder.num_patches, m.hidden_size, m.num_heads)
    assert stack == (tag == "dit_small_hd64w")          # hd72's 64 tokens at head dim 72: the per-block DitBlockFn route, which only has to stay correct
    # the training route with trainable weights: the full backward
    xa = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        out_a = m(xa, t, y)
    (out_a.float() * dy).sum().backward()
    # the frozen model: dx only, no weight-gradient entry point reached
    with monkeypatch.context() as mp:
        if stack:
            _forbid_weight_gradients(mp)
        xb = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            out_b = fz(xb, t, y)
            dx = torch.autograd.grad((out_b.float() * dy).sum(), xb)[0]
            keep = dx.clone()
            xc = x.clone().requires_grad_(True)
            out_c = fz(xc, t, y)                                       # the reference's second call: the same bits as the VJP's forward
            dx2 = torch.autograd.grad((out_c.float() * dy.flip(0)).sum(), xc)[0]
    assert torch.equal(out_b, out_a) and torch.equal(out_c, out_b)
    assert torch.equal(dx, xa.grad)
    assert torch.equal(dx, keep) and not torch.equal(dx2, dx)          # a second VJP leaves the first result alone
    assert all(p.grad is None for p in fz.parameters())
    # dx against the reference's f32 capture by the bf16-site criterion of test_gpu_dit.py
    names = [n for n, _ in m.named_parameters()]
    po = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for n in names:
        po[n].requires_grad_(True)
    xo = g.t("x").clone().requires_grad_(True)
    yo = R.lightningdit_forward(xo, g.t("t"), torch.from_numpy(np.asarray(g["y"])), po, CFGS[tag]["num_heads"], CFGS[tag]["patch_size"], q=R.bf16_round)
    yo.backward(g.t("dy"))
    e_hip, e_orc = _rl2(dx.cpu(), g.t("dx")), _rl2(xo.grad, g.t("dx"))
    print(f"{tag} frozen dx: rel-L2 to the f32 reference -- HIP {e_hip:.2e}, bf16-site oracle {e_orc:.2e}")
    assert e_hip < 1.15 * e_orc + 1e-3
    # without an input gradient the frozen model keeps the inference route
    with torch.autocast("cuda", dtype=BF):
        want = LF.forward_inference(fz, x, t, y)
        assert torch.equal(fz(x, t, y), want)
        with torch.no_grad():
            assert torch.equal(fz(x.clone().requires_grad_(True), t, y), want)


def _xl1(seed=0):
    from dmvae_amd.train import _randomised_dit
    torch.manual_seed(seed)
    return _randomised_dit(DEV).eval()          # eval: no label dropout, so two calls see the same conditioning


def test_dit_xl1_input_vjp_equals_full_backward(monkeypatch):
    """At production width (LightningDiT-XL/1, 256 tokens, B = 8: split-K GEMMs, the tight attention backward, DitStackFn) the dx-only route's dx is the full
    backward's dx bit for bit."""
    m = _xl1()
    fz = _frozen_copy(m)
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(8, 32, 16, 16, device=DEV, generator=g)
    t = torch.rand(8, device=DEV, generator=g)
    y = torch.randint(0, 1000, (8,), device=DEV, generator=g)
    eps = torch.randint(2, x.size(), dtype=torch.float, device=DEV, generator=g) * 2 - 1
    xa = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        out_a = m(xa, t, y)
    (out_a * eps).sum().backward()
    m.zero_grad(set_to_none=True)
    with monkeypatch.context() as mp:
        _forbid_weight_gradients(mp)
        xb = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            out_b = fz(xb, t, y)
            dx = torch.autograd.grad((out_b * eps).sum(), xb)[0]
    assert torch.equal(out_a, out_b) and torch.equal(dx, xa.grad) and dx.abs().max() > 0
    assert all(p.grad is None for p in fz.parameters())


def test_sample_ode_likelihood_dit_xl1():
    """`Sampler(create_transport()).sample_ode_likelihood()` at every default with LightningDiT-XL/1 (random weights, B = 8) under autocast(bf16): finite
    logp, counters recorded, a seeded rerun bit-identical."""
    from dmvae_amd.transport import Sampler, create_transport
    m = _xl1(1).requires_grad_(False)
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(8, 32, 16, 16, device=DEV, generator=g)
    y = torch.randint(0, 1000, (8,), device=DEV, generator=g)
    fn = Sampler(create_transport()).sample_ode_likelihood()
    runs = []
    for _ in range(2):
        torch.manual_seed(123)
        with torch.autocast("cuda", dtype=BF):
            logp, z = fn(x, m.forward, y=y)
        o = fn.ode
        runs.append((logp, z, (o.nfe, o.n_accepted, o.n_rejected)))
    (la, za, ca), (lb, zb, cb) = runs
    assert la.shape == (8,) and la.dtype == torch.float32 and torch.isfinite(la).all() and torch.isfinite(za).all()
    assert ca[0] >= 8 and ca[0] == 2 + 6 * (ca[1] + ca[2]) and ca[1] >= 1
    assert torch.equal(la, lb) and torch.equal(za, zb) and ca == cb
    d = x[0].numel()
    print(f"likelihood, DiT-XL/1 random weights: NFE {ca[0]} (accepted {ca[1]}, rejected {ca[2]}), bits/dim {(-la / d / np.log(2)).tolist()}")
