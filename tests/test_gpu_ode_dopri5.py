"""The adaptive dopri5 ODE sampler on the MI355X (-m gpu): `Sampler.sample_ode()` with the reference's defaults (transport.py:356-407 ->
torchdiffeq.odeint, integrators.py:79-118) on a CUDA f32 state.  Its kernels (csrc/sampler.hip: ode_rk_combine / ode_error_ratio / ode_dense_output)
against their definitions written with tensor ops, the whole integrator against its composed route, the float64 restatement of tests/dopri5_spec.py
and an exact solution, then the reference's call sites: LightningDiT under autocast(bf16), SamplePipeline(mode="ODE"), the toy's [B, 2, 1, 1] state."""
import os
import warnings

import numpy as np
import pytest
import torch

import dopri5_spec as S
from test_oracle_dopri5 import ATOL, RTOL, lam_problem, shifted_grid

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SIZES = (14, 4097, 25 * 32 * 16 * 16)


def _bf(v):
    return float(torch.tensor(v, dtype=torch.float32).to(BF))


def _terms(n, nk, kdtype, seed, offset=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ks = [(torch.randn(n + offset, device=DEV, generator=g) * (1 + j)).to(kdtype)[offset:] for j in range(nk)]
    cs = [float(np.float32(v)) for v in (torch.rand(nk, generator=torch.Generator().manual_seed(seed)) * 0.4 - 0.2).tolist()]
    y0 = (torch.randn(n + offset, device=DEV, generator=g) * 3)[offset:]
    return y0, ks, cs


def _sum_f32(ks, cs):
    s = None
    for c, k in zip(cs, ks):
        s = c * k.float() if s is None else s + c * k.float()
    return s


def _sum_bf16(ks, cs):
    s = None
    for c, k in zip(cs, ks):
        p = _bf(c) * k.to(BF).float()
        s = p if s is None else s + p
    return s.to(BF).float()


@pytest.mark.parametrize("kdtype", [torch.float32, BF])
@pytest.mark.parametrize("n", SIZES)
def test_rk_combine_bit_exact(n, kdtype):
    """round_bf16 = 0: the f32 sum written in torch, to the bit; round_bf16 = 1: its own definition (bf16 weights and k, f32 sum, bf16 result) to the bit.
    With and without y0, for 1..7 terms; offset views (no quads: the scalar path) give the same bits."""
    from dmvae_amd import ops
    for nk in range(1, 8):
        for offset in (0, 1):
            if offset and n > 5000:
                continue
            y0, ks, cs = _terms(n, nk, kdtype, 100 * nk + n % 97 + offset, offset)
            s = _sum_f32(ks, cs)
            assert torch.equal(ops.ode_rk_combine(y0, ks, cs), y0 + s), (nk, offset)
            assert torch.equal(ops.ode_rk_combine(None, ks, cs), s), (nk, offset)
            sb = _sum_bf16(ks, cs)
            assert torch.equal(ops.ode_rk_combine(y0, ks, cs, round_bf16=True), y0 + sb), (nk, offset)


def test_rk_combine_bf16_form_is_the_autocast_matmul():
    """The round_bf16 sum is what torch.matmul(k, coef) under autocast(bf16) returns -- torchdiffeq's k.matmul(beta_i * dt) -- within 1 bf16 ulp."""
    from dmvae_amd import ops
    for nk in (2, 5, 7):
        _, ks, cs = _terms(4097, nk, torch.float32, 7 + nk)
        with torch.autocast("cuda", dtype=BF):
            m = torch.stack(ks, -1).matmul(torch.tensor(cs, device=DEV))
        assert m.dtype == BF
        got = ops.ode_rk_combine(None, ks, cs, round_bf16=True)
        mag = torch.maximum(got.abs(), m.float().abs()).clamp_min(1e-30)
        ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
        assert ((got - m.float()).abs() <= ulp).all(), nk


@pytest.mark.parametrize("n", SIZES)
def test_error_ratio_deterministic_and_accurate(n):
    """mean(e^2) of the error test: the same bits on every run, within 1e-6 relative of the float64 value; the non-finite flag follows the data of y1."""
    from dmvae_amd import ops
    y0, ks, cs = _terms(n, 7, torch.float32, n % 1000)
    y1 = y0 + 0.01 * ks[3]
    cs = [c * 1e-3 for c in cs]
    runs = [ops.ode_error_ratio(y0, y1, ks, cs, ATOL, RTOL).clone() for _ in range(3)]
    assert all(torch.equal(r, runs[0]) for r in runs)
    k64 = [k.double().cpu() for k in ks]
    err = sum(float(np.float32(c)) * k for c, k in zip(cs, k64))
    tol = ATOL + RTOL * torch.maximum(y0.double().cpu().abs(), y1.double().cpu().abs())
    want = ((err / tol) ** 2).mean().item()
    assert abs(runs[0][0].item() - want) <= 1e-6 * want, (runs[0][0].item(), want)
    assert runs[0].view(torch.int32)[1].item() == 0
    err_out = torch.empty_like(y0)
    ops.ode_error_ratio(y0, y1, ks, cs, ATOL, RTOL, err_out=err_out)
    assert torch.equal(err_out, _sum_f32(ks, cs))
    rb = ops.ode_error_ratio(y0, y1, ks, cs, ATOL, RTOL, round_bf16=True, err_out=err_out)
    assert torch.equal(err_out, _sum_bf16(ks, cs))
    eb = err_out.double().cpu() / tol
    assert abs(rb[0].item() - (eb ** 2).mean().item()) <= 1e-6 * (eb ** 2).mean().item()
    for bad in (float("inf"), float("nan"), -float("inf")):
        for where in (0, n - 1):
            y1b = y1.clone()
            y1b[where] = bad
            assert ops.ode_error_ratio(y0, y1b, ks, cs, ATOL, RTOL).view(torch.int32)[1].item() == 1, (bad, where)


@pytest.mark.parametrize("n", SIZES)
def test_dense_output_bit_exact_vs_composed(n):
    from dmvae_amd import ops
    from dmvae_amd import transport as T
    y0, ks, _ = _terms(n, 4, torch.float32, 3 + n % 13)
    y1, ymid, f0, f1 = y0 + 0.1 * ks[0], y0 + 0.05 * ks[1], ks[2], ks[3]
    comp = T._Dopri5(None, y0, atol=ATOL, rtol=RTOL, fused=False, round_bf16=False)
    comp.k[0].copy_(f0)
    comp.k[6].copy_(f1)
    for dt, x in ((0.0371, 0.0), (0.0371, 0.3791), (0.21, 1.0), (0.013, 0.91)):
        want = comp.dense(y0, y1, ymid, dt, x, torch.empty_like(y0))
        assert torch.equal(ops.ode_dense_output(y0, y1, ymid, f0, f1, dt, x), want), (dt, x)
        f0b, f1b = f0.to(BF), f1.to(BF)                                # bf16 f0 / f1 read as their exact f32 values
        assert torch.equal(ops.ode_dense_output(y0, y1, ymid, f0b, f1b, dt, x), ops.ode_dense_output(y0, y1, ymid, f0b.float(), f1b.float(), dt, x))
    assert torch.equal(ops.ode_dense_output(y0, y1, ymid, f0, f1, 0.05, 0.0), y0)


def _analytic_model(x, t, **kw):
    """The velocity of lam_problem(): (-1 + 6 cos 20t) x."""
    return (torch.cos(20 * t) * 6 - 1).view(-1, *([1] * (x.dim() - 1))) * x


def _sample(fn, z, model, fused, amp=False, **kw):
    from dmvae_amd import transport as T
    T.FUSED_STATE_UPDATE = fused
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=BF, enabled=amp):
            out = fn(z, model, **kw)
        o = fn.__self__
        return out, (o.nfe, o.n_accepted, o.n_rejected)
    finally:
        T.FUSED_STATE_UPDATE = True


@pytest.mark.parametrize("amp", [False, True])
def test_integrator_fused_composed_spec_and_exact(amp):
    """An analytic drift on the device (y' = (-1 + 6 cos 20t) y, 6 of 16 steps rejected): the fused and composed routes take the same steps and agree to
    1e-6; without autocast they take the float64 spec's steps (no error ratio of the spec within 1e-3 of 1) and stay within the tolerance of the exact solution."""
    from dmvae_amd.transport import Sampler, create_transport
    z = (torch.linspace(-1, 1, 3 * 7 * 5, device=DEV) + 0.05).view(3, 7, 5)
    fn = Sampler(create_transport(time_dist_shift=2.5)).sample_ode()
    fused, cf = _sample(fn, z, _analytic_model, True, amp)
    comp, cc = _sample(fn, z, _analytic_model, False, amp)
    assert cf == cc and cf[0] == 2 + 6 * (cf[1] + cf[2]) and cf[2] > 0
    assert fused.shape == (50, 3, 7, 5) and torch.equal(fused[0], z)
    assert ((fused - comp).abs().max() / comp.abs().max()).item() < 1e-6
    if amp:
        return
    ts = shifted_grid()
    lam, sol = lam_problem()
    want, steps, nfe = S.solve(lambda t, y: lam(t) * y, z.double().cpu().numpy(), ts, ATOL, RTOL)
    assert min(abs(s[2] - 1) for s in steps) > 1e-3
    assert cf == (nfe, sum(s[3] for s in steps), sum(not s[3] for s in steps))
    got = fused.double().cpu().numpy()
    assert np.abs(got - want).max() < 1e-5 * np.abs(want).max()
    ex = np.stack([sol(z.double().cpu().numpy(), t, ts[0]) for t in ts])
    assert np.abs(got - ex).max() < 10 * (ATOL + RTOL * np.abs(ex).max())


def test_sample_ode_defaults_on_the_hip_dit():
    """`Sampler(create_transport(time_dist_shift=2.5)).sample_ode()` -- every default, dopri5 -- with LightningDiT on the HIP route under autocast(bf16), as
    sample_50k.py --mode ODE runs it: [50, ...] stacked like odeint, out[0] is z, deterministic, and nearer a 400-step rk4 solution than 50-step Euler is."""
    from dmvae_amd.transport import Sampler, create_transport
    from test_oracle_sampler import small_dit
    m = small_dit(5).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    z = torch.randn(3, 8, 8, 8, device=DEV, generator=g)
    y = torch.tensor([1, 4, 9], device=DEV)
    sampler = Sampler(create_transport(time_dist_shift=2.5))
    fn = sampler.sample_ode()
    a, counts = _sample(fn, z, m.forward, True, True, y=y)
    b, counts_b = _sample(fn, z, m.forward, True, True, y=y)
    assert a.shape == (50, 3, 8, 8, 8) and a.dtype == torch.float32 and torch.isfinite(a).all()
    assert torch.equal(a[0], z) and torch.equal(a, b) and counts == counts_b
    print(f"dopri5 on the small DiT: NFE {counts[0]}, accepted {counts[1]}, rejected {counts[2]}")
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        rk4 = sampler.sample_ode(sampling_method="rk4", num_steps=401)(z, m.forward, y=y)[-1].float()
        eul = sampler.sample_ode(sampling_method="euler", num_steps=50)(z, m.forward, y=y)[-1].float()
    d_dopri, d_euler = (a[-1] - rk4).norm().item(), (eul - rk4).norm().item()
    assert d_dopri < d_euler, (d_dopri, d_euler)


def _pipeline_models():
    from dmvae_amd.models.lightningdit import LightningDiT
    from dmvae_amd.models.vae import VAE
    torch.manual_seed(4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = VAE(z_channels=32, model_size="base", encoder_kwargs=dict(embed_dim=256, depth=1, num_heads=4)).to(DEV).eval()
    dit = LightningDiT(input_size=16, patch_size=1, in_channels=32, hidden_size=192, depth=2, num_heads=3, num_classes=10).to(DEV).eval()
    with torch.no_grad():
        for blk in dit.blocks:
            blk.adaLN_modulation[1].weight.normal_(0, 0.02)
        dit.final_layer.linear.weight.normal_(0, 0.05)
    return dit, vae


def test_sample_pipeline_ode_dopri5(tmp_path, monkeypatch):
    """SamplePipeline(mode="ODE", sampling_method="dopri5"): the same uint8 images with and without the graphed DiT forward (captured once per batch shape,
    not per step), and run() writes the file layout of the SDE pipeline."""
    from dmvae_amd.models import lightningdit_fast as fast
    from dmvae_amd.sample import SamplePipeline
    dit, vae = _pipeline_models()
    captures = []
    orig = fast.GraphedInference.__init__
    monkeypatch.setattr(fast.GraphedInference, "__init__", lambda self, *a, **k: (captures.append(1), orig(self, *a, **k))[1])
    z = torch.randn(5, 32, 16, 16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    y = torch.tensor([0, 1, 2, 3, 4], device=DEV)
    imgs = []
    for use_graph in (True, False):
        pipe = SamplePipeline(dit, vae, mode="ODE", sampling_method="dopri5", latent_mean=0.0685, latent_scale=0.1763, time_dist_shift=2.5, use_graph=use_graph)
        u8, tok = pipe.images_uint8(z, y)
        imgs.append(u8)
        if use_graph:
            u8_again, _ = pipe.images_uint8(z, y)
            assert torch.equal(u8_again, u8) and len(captures) == 1
            assert pipe.sample_fn.__self__.nfe > 2
    assert torch.equal(imgs[0], imgs[1]) and imgs[0].shape == (5, 256, 256, 3) and torch.isfinite(tok).all()
    layouts = []
    for mode, method in (("ODE", "dopri5"), ("SDE", "Euler")):
        d = tmp_path / mode
        pipe = SamplePipeline(dit, vae, mode=mode, sampling_method=method, num_sampling_steps=50 if mode == "ODE" else 6, latent_mean=0.0685,
                              latent_scale=0.1763, time_dist_shift=2.5)
        assert pipe.run(str(d), per_proc_batch_size=5, num_fid_samples=40, num_classes=10, rank=1, world_size=2, max_iterations=1) == 5
        layouts.append(sorted(os.listdir(d)))
    assert layouts[0] == layouts[1] and len(layouts[0]) == 5


def test_toy_state_one_token_route():
    """The 2-D toy's state [B, 2, 1, 1] (toy_example_2d/train_diffusion.py:308-312; n = 2B, not a multiple of 4) through LightningDiT-Mini/1's one-token
    route under autocast(bf16): fused and composed routes take the same steps and agree to 1e-6."""
    from dmvae_amd.models.lightningdit import LightningDiT_models
    from dmvae_amd.transport import Sampler, create_transport
    from oracle.detweights import det_fill_
    m = LightningDiT_models["LightningDiT-Mini/1"](input_size=1, in_channels=2, num_classes=1)
    det_fill_(m, 21, skip=("pos_embed",))
    m = m.to(DEV).eval()
    z = torch.randn(37, 2, 1, 1, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    y = torch.zeros(37, dtype=torch.long, device=DEV)
    fn = Sampler(create_transport(time_dist_shift=2.5)).sample_ode()
    a, ca = _sample(fn, z, m.forward, True, True, y=y)
    b, cb = _sample(fn, z, m.forward, False, True, y=y)
    assert a.shape == (50, 37, 2, 1, 1) and torch.isfinite(a).all() and torch.equal(a[0], z)
    assert ca == cb, (ca, cb)
    assert ((a - b).abs().max() / b.abs().max()).item() < 1e-6
