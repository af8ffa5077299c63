"""The rest of the Linear / velocity sampler on the MI355X (-m gpu): the Heun step's three kernels and the "Tweedie" / "Euler" last-step kernel
(csrc/sampler.hip) bit-exact against the reference's f32 elementwise graph evaluated on the CPU from the same inputs, `sample_sde` on the small HIP LightningDiT
bit-identical between the kernel route and the tensor-op composition, and autoguidance: the combine kernel against the composition, its graph and the pipeline.

Bit-exactness needs no tolerance: every operation is an IEEE f32 (or bf16-rounded) one, nothing is contracted, and the scalars are formed by the host exactly as
the reference's broadcast graph forms them.  Where a coefficient is infinite (SBDM at t = 0: 1 / t; Tweedie at t = 0: x / 0) the reference's result holds NaNs,
which compare unequal to themselves: `_same` asks for NaN at the same places and equal values everywhere else.

Shapes, for every kernel: (3, 1, 1, 1) -- scalar tail only; (1, 2, 3, 7) -- quads and a tail; (5, 8, 6, 6); the same through a view that starts one element
into its buffer, whose pointers forbid quads; and (1, 2048 * 256 * 4 + 7), seven elements past what the launcher's grid cap (2048 workgroups of 256 threads,
one quad each) covers in one sweep, so the grid-stride loop runs twice and a tail follows."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import ref_cpu as R
from test_oracle_sampler import _kw, small_dit
from test_sampler_methods_host import autoguidance_models

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SHAPES = [((3, 1, 1, 1), 0), ((1, 2, 3, 7), 0), ((5, 8, 6, 6), 0), ((5, 8, 6, 6), 1), ((1, 2048 * 256 * 4 + 7), 0)]
FORMS = [("sigma", 1.0), ("linear", 0.7), ("SBDM", 1.0)]
TIMES = [0.0, 0.5139, 0.96]
DT = torch.linspace(0, 0.96, 250)[1] - torch.linspace(0, 0.96, 250)[0]


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """x, w, v1, v2 (f32, CPU) for one shape: drawn once, shared by every case, never written."""
    g = torch.Generator().manual_seed(sum(shape))
    return tuple(torch.randn(shape, generator=g) * s for s in (1.7, 1.0, 2.0, 2.0))


def _dev(t, offset=0):
    """`t` on the device, contiguous; offset 1: a view that starts one element into its buffer (4 bytes for f32, 2 for bf16: no quad is aligned)."""
    if not offset:
        return t.to(DEV)
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    out = buf[offset:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 8 != 0
    return out


def _same(got, want):
    got, nan = got.cpu(), want.isnan()
    zero = torch.zeros((), dtype=want.dtype)
    return got.dtype == want.dtype and torch.equal(got.isnan(), nan) and torch.equal(torch.where(nan, zero, got), torch.where(nan, zero, want))


def _scalars(t, form, norm):
    """(rar, var, diff, sqrt(2 diff)) at the 0-d f32 time t, the way `transport.sde._coeffs` forms them."""
    from dmvae_amd.transport import ICPlan
    ps, te = ICPlan(), t.view(1, 1)
    rar, var = ps._score_coeffs(te)
    diff = ps.compute_diffusion(te, te.view(1), form=form, norm=norm)
    return float(rar), float(var), float(diff), float(torch.sqrt(2 * diff))


@pytest.mark.parametrize("vdtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("tval", TIMES)
@pytest.mark.parametrize("form,norm", FORMS)
def test_heun_step_kernels_bit_exact(form, norm, tval, vdtype):
    """ops.sde_heun_perturb / sde_heun_predict / sde_heun_correct == the reference's Heun step (integrators.py:37-48 over transport.py:253-256 and path.py:74-89),
    written out op by op on the CPU; each kernel is fed the reference's own intermediate values, so each is checked on its own."""
    from dmvae_amd import ops
    t = torch.tensor(tval, dtype=torch.float32)
    rar, var, diff, sq2d = _scalars(t, form, norm)
    rar2, var2, diff2, _ = _scalars(t + DT, form, norm)
    for shape, off in SHAPES:
        x, w, v1, v2 = _inputs(shape)
        v1, v2 = v1.to(vdtype), v2.to(vdtype)
        # the reference's graph
        t_cur = torch.ones(shape[0]) * t
        dw = w * torch.sqrt(DT)
        diffusion = R.icplan_diffusion(R.expand_t(t_cur, x), form, norm)
        xhat = x + torch.sqrt(2 * diffusion) * dw
        k1 = R.sde_drift_from_velocity(v1, xhat, t_cur, form, norm)
        xp = xhat + DT * k1
        k2 = R.sde_drift_from_velocity(v2, xp, t_cur + DT, form, norm)
        x_new = xhat + 0.5 * DT * (k1 + k2)
        # the kernels, each from the reference's inputs
        d = lambda a: _dev(a, off)
        assert _same(ops.sde_heun_perturb(d(x), d(w), sq2d, float(torch.sqrt(DT))), xhat), (shape, off, "perturb")
        got_k1, got_xp = ops.sde_heun_predict(d(xhat), d(v1), rar, var, diff, float(DT))
        assert _same(got_k1, k1) and _same(got_xp, xp), (shape, off, "predict")
        assert _same(ops.sde_heun_correct(d(xhat), d(xp), d(k1), d(v2), rar2, var2, diff2, float(0.5 * DT)), x_new), (shape, off, "correct")


@pytest.mark.parametrize("vdtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("form,norm,tval", [("linear", 0.7, 0.9599), ("SBDM", 1.0, 0.3)])
def test_euler_step_kernel_bit_exact_at_every_shape(form, norm, tval, vdtype):
    """ops.sde_euler_step for a velocity model == the reference's Euler-Maruyama step and "Mean" last step (oracle.ref_cpu.sde_euler_step /
    sde_drift_from_velocity on the CPU, as tests/test_gpu_sampler.py compares them at one shape) at every shape of SHAPES and at (1, 2, 3, 7) through the
    offset view: 42 elements, no multiple of four, behind pointers that forbid quads.  The entry point takes any n > 0."""
    import ctypes
    from dmvae_amd import _lib, ops
    t = torch.tensor(tval, dtype=torch.float32)
    rar, var, diff, sq2d = _scalars(t, form, norm)
    for shape, off in SHAPES + [((1, 2, 3, 7), 1)]:
        x, w, v, _ = _inputs(shape)
        v = v.to(vdtype)
        tv = torch.ones(shape[0]) * t
        x_ref, mean_ref = R.sde_euler_step(x, v.float(), w, tv, DT, form, norm)
        d = lambda a: _dev(a, off)
        out, mean = ops.sde_euler_step(d(x), d(v), d(w), rar, var, diff, float(DT), sq2d, float(torch.sqrt(DT)), need_mean=True)
        assert _same(out, x_ref) and _same(mean, mean_ref), (shape, off, "step")
        last, none = ops.sde_euler_step(d(x), d(v), None, rar, var, diff, 0.04, 0.0, 0.0)
        assert none is None and _same(last, x + R.sde_drift_from_velocity(v.float(), x, tv, form, norm) * 0.04), (shape, off, "mean")
    src, dst = torch.zeros(5, device=DEV), torch.ones(5, device=DEV)          # the C entry itself: n = 5 passes the argument check
    torch.cuda.synchronize()
    p, q = ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr())
    assert _lib.lib().dmvae_sde_euler_step(p, p, 0, None, None, q, 5, 0.5, 0.5, 0.5, 0.1, 0.0, 0.0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, src)                                              # x = v = 0: the mean is 0


@pytest.mark.parametrize("vdtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("tval", TIMES)
@pytest.mark.parametrize("mode,h", [("Tweedie", 0.04), ("Euler", 0.04), ("Euler", 0.1)])
def test_last_step_kernel_bit_exact(mode, h, tval, vdtype):
    """ops.sde_last_step == the reference's "Tweedie" and "Euler" last steps (transport.py:279-288) on the CPU, the model output in the type the model returns
    it in: a bf16 v times the Python float last_step_size stays bf16 before it meets the f32 state.  Neither step involves the diffusion coefficient, so the
    diffusion forms do not enter; t = 0 makes Tweedie's alpha zero (infinities and NaNs, at the reference's places)."""
    from dmvae_amd import ops
    from dmvae_amd.transport import ICPlan
    ps = ICPlan()
    t1 = torch.tensor(tval, dtype=torch.float32)
    for shape, off in SHAPES:
        x, _, v, _ = _inputs(shape)
        v = v.to(vdtype)
        t = torch.ones(shape[0]) * t1
        if mode == "Tweedie":
            alpha, sigma = ps.compute_alpha_t, ps.compute_sigma_t
            want = x / alpha(t)[0][0] + (sigma(t)[0][0] ** 2) / alpha(t)[0][0] * ps.get_score_from_velocity(v, x, t)
            te = t[:1].view(1, 1)
            rar, var = ps._score_coeffs(te)
            a = alpha(te)[0]
            got = ops.sde_last_step(_dev(x, off), _dev(v, off), ops.LAST_STEP_TWEEDIE, a=float(a), c=float((sigma(te)[0] ** 2) / a), rar=float(rar), var=float(var))
        else:
            want = x + v * h
            got = ops.sde_last_step(_dev(x, off), _dev(v, off), ops.LAST_STEP_EULER, h=h)
        assert want.dtype == torch.float32 and _same(got, want), (shape, off)


def test_new_sampler_ops_validate_inputs():
    from dmvae_amd import ops
    x = torch.zeros(2, 3, 2, 2, device=DEV)
    with pytest.raises(ValueError):
        ops.sde_heun_perturb(x, x[:1], 1.0, 1.0)                           # shapes differ
    with pytest.raises(TypeError):
        ops.sde_heun_predict(x.to(BF), x, 0.5, 0.5, 0.5, 0.1)             # the state is f32
    with pytest.raises(TypeError):
        ops.sde_heun_correct(x, x, x, x.double(), 0.5, 0.5, 0.5, 0.05)    # v: bf16 or f32
    with pytest.raises(ValueError):
        ops.sde_last_step(x, x.transpose(2, 3), ops.LAST_STEP_EULER, h=0.04)      # not contiguous
    with pytest.raises(ValueError):
        ops.sde_last_step(x, x, 2)
    t = torch.zeros(2, device=DEV)
    with pytest.raises(TypeError):
        ops.autoguidance_combine(x, x.to(BF), 3, 2.5, t)                   # the two outputs in one type
    with pytest.raises(ValueError):
        ops.autoguidance_combine(x, x, 4, 2.5, t)                          # more channels than the outputs have
    with pytest.raises(ValueError):
        ops.autoguidance_combine(x, x, 3, 2.5, t.cpu())                    # t on the CPU
    with pytest.raises(ValueError):
        ops.autoguidance_combine(x, x[:, :, :1], 3, 2.5, t)                # ag of another spatial size
    with pytest.raises(ValueError):
        ops.autoguidance_combine(x, x, 3, 2.5, t, out=torch.zeros(2, 3, 2, 2, device=DEV))       # out is [2n, k, H, W]


def _run_sde(g, fused, model_fn, z, y):
    from dmvae_amd import transport as T
    fn = T.Sampler(T.create_transport("Linear", "velocity", None, None, None, time_dist_shift=2.5)).sample_sde(**_kw(g))
    T.FUSED_STATE_UPDATE = fused
    try:
        torch.manual_seed(int(g["seed"]))
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            return torch.stack(fn(z, model_fn, y=y)).float().cpu()
    finally:
        T.FUSED_STATE_UPDATE = True


def test_heun_trajectory_bit_identical_to_the_composition():
    """`sample_sde(sampling_method="Heun")` of the sampler_heun_linear_mean fixture with the small LightningDiT on the HIP kernels under autocast(bf16): every state
    of the kernel route equals the tensor-op composition's (same noise stream).  The coefficients are IEEE arithmetic on either side but for one function: the
    composition takes sqrt(2 diffusion) with ATen's device sqrt, which is not correctly rounded on this stack (about one f32 input in six is an ulp off the
    host's); the kernel route takes the host's, as the CPU reference does.  At this fixture's five step times the two agree, and the grid is fixed, so the
    comparison is exact and repeatable; on a longer grid the routes part at the first time whose 2 diffusion is such an input (tools/bench_sampler_methods.py)."""
    g = load_golden("sampler_heun_linear_mean")
    assert _kw(g)["sampling_method"] == "Heun"
    m = small_dit(g["dit_seed"]).to(DEV)
    z, y = g.t("z").to(DEV), torch.from_numpy(np.asarray(g["y"])).to(DEV)
    fused, plain = _run_sde(g, True, m.forward, z, y), _run_sde(g, False, m.forward, z, y)
    assert fused.shape == g.t("xs").shape and torch.isfinite(fused).all()
    assert torch.equal(fused, plain)


@pytest.mark.parametrize("tag,last", [("sampler_euler_decreasing_euler", "Euler"), ("sampler_euler_incdec_tweedie", "Tweedie")])
def test_last_state_bit_identical_to_the_composition(tag, last):
    """The "Euler" and "Tweedie" last states of the two fixtures that use them: `Sampler._last_step` on the kernel against its composition, from the SAME state --
    the one the sampler reaches before its last step.  (These fixtures' diffusion forms take cos / sin, which the kernel route evaluates on the host and the
    composition on the device, so two whole runs differ in the last digits before the last step is reached: tests/test_gpu_sampler.py holds them to 5e-3.)"""
    from dmvae_amd import transport as T
    g = load_golden(tag)
    kw = _kw(g)
    assert kw["last_step"] == last
    m = small_dit(g["dit_seed"]).to(DEV)
    z, y = g.t("z").to(DEV), torch.from_numpy(np.asarray(g["y"])).to(DEV)
    x = _run_sde(g, True, m.forward, z, y)[-2].to(DEV)
    sampler = T.Sampler(T.create_transport("Linear", "velocity", None, None, None, time_dist_shift=2.5))
    sde_drift, _ = sampler._sde_diffusion_and_drift(diffusion_form=kw["diffusion_form"], diffusion_norm=kw["diffusion_norm"])
    t1 = 1 - kw["last_step_size"]
    t = torch.ones(z.size(0), device=DEV) * t1
    outs = []
    step = sampler._last_step(sde_drift, last_step=last, last_step_size=kw["last_step_size"], t1=t1,
                              fused=(sampler.transport.path_sampler, kw["diffusion_form"], kw["diffusion_norm"]))
    for fused in (True, False):
        T.FUSED_STATE_UPDATE = fused
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=BF):
                outs.append(step(x, t, m.forward, y=y))
        finally:
            T.FUSED_STATE_UPDATE = True
    assert outs[0].dtype == torch.float32 and torch.isfinite(outs[0]).all() and not torch.equal(outs[0], x)
    assert torch.equal(outs[0], outs[1])


def _compose(eps, ag, k, scale, t, interval):
    """lightningdit.py:459-465 on two outputs."""
    eps, ag = eps[:, :k], ag[:, :k]
    if t[0] >= interval[0] and t[0] <= interval[1]:
        eps = ag + scale * (eps - ag)
    return torch.cat([eps, eps], dim=0)


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "f32"])
def test_autoguidance_combine_kernel_bit_exact(dtype):
    """ops.autoguidance_combine == the reference's expression on the CPU in the same type: quads ((2, 8, 8, 8), all channels), the scalar tail with fewer guided
    channels than the outputs hold and outputs of different widths ((3, 5, 3, 3) against 7 channels, k = 3), the offset view, and more than the grid cap
    (2048 workgroups of 256 threads) covers in one sweep, as scalars ((1, 1, 1449, 1449): an odd 2099601 elements) and as quads ((1, 1, 1024, 2052)); t inside, on both edges of, below and above the interval, and the default interval."""
    from dmvae_amd import ops
    g = torch.Generator().manual_seed(5)
    interval, scale = (0.25, 0.75), 2.5
    for (n, c, h, w), c_ag, k, off in (((2, 8, 8, 8), 8, 8, 0), ((3, 5, 3, 3), 7, 3, 0), ((2, 8, 8, 8), 8, 8, 1), ((1, 1, 1449, 1449), 1, 1, 0),
                                       ((1, 1, 1024, 2052), 1, 1, 0)):
        eps, ag = (torch.randn(n, c, h, w, generator=g) * 2).to(dtype), (torch.randn(n, c_ag, h, w, generator=g) * 2).to(dtype)
        eps_d, ag_d = _dev(eps, off), _dev(ag, off)
        for t0 in (0.5, 0.25, 0.75, 0.2, 0.9):
            t = torch.tensor([t0, 0.4, 0.6])
            want = _compose(eps, ag, k, scale, t, interval)
            got = ops.autoguidance_combine(eps_d, ag_d, k, scale, t.to(DEV), interval)
            assert got.shape == want.shape == (2 * n, k, h, w) and _same(got, want), (n, c, h, w, off, t0)
        assert _same(ops.autoguidance_combine(eps_d, ag_d, k, scale, t.to(DEV)), torch.cat([eps[:, :k]] * 2))          # (-1e4, -1e4): never inside
        assert _same(ops.autoguidance_combine(eps_d, ag_d, k, scale, torch.tensor([0.5], dtype=torch.float64, device=DEV), interval),
                     _compose(eps, ag, k, scale, torch.tensor([0.5]), interval))


@pytest.fixture(scope="module")
def ag_models():
    g = load_golden("autoguidance")
    m, guide = autoguidance_models(g)
    return g, m.to(DEV).requires_grad_(False), guide.to(DEV).requires_grad_(False)


def test_autoguidance_kernel_route_equals_the_composition_and_its_graph(ag_models):
    """With both small LightningDiTs on the HIP inference route under autocast(bf16): `forward_with_autoguidance` (two forwards + one kernel) equals
    `forward_with_autoguidance_composed` bit for bit inside and outside the interval; `GraphedInferenceAutoguidance`, captured once, follows a replayed t across the
    interval's edge without re-capture and returns the eager call's bits; keywords that differ from the captured ones are an error."""
    from dmvae_amd.models import lightningdit_fast as fast
    g, m, guide = ag_models
    x, y = g.t("x").to(DEV), torch.from_numpy(np.asarray(g["y"])).to(DEV)
    scale, interval = float(g["cfg_scale"]), tuple(float(v) for v in g["interval"])
    n = x.shape[0] // 2
    kw = dict(cfg_scale=scale, additional_model_forward=guide.forward, cfg_interval=interval)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        assert m._takes_inference_route(x[:n])
        gi = fast.GraphedInferenceAutoguidance(m, x, torch.zeros(2 * n, device=DEV), y, **kw)
        graph = gi.graph
        gen = torch.Generator(device=DEV).manual_seed(3)
        seen = []
        for i in range(int(g["n_cases"])):
            t = g.t(f"t_{i}").to(DEV)
            xi = x + 0.1 * i * torch.randn(x.shape, device=DEV, generator=gen)
            eager = m.forward_with_autoguidance(xi, t, y, **kw)
            assert eager.dtype == BF and eager.shape == (2 * n, m.in_channels, *x.shape[2:]) and torch.equal(eager[:n], eager[n:])
            assert torch.equal(eager, m.forward_with_autoguidance_composed(xi, t, y, **kw)), i
            own = m.forward(xi[:n], t[:n], y[:n])[:, :m.in_channels]
            seen.append(bool(torch.equal(eager[:n], own)))
            assert torch.equal(gi(xi, t, y, **kw), eager), i
        assert seen == [False, False, False, True, True]      # guided inside and on the edges, this model's own output outside
        assert gi.graph is graph                               # one capture served every t
        assert torch.equal(gi(xi, t, y), eager)                # keywords left out: the captured ones
        with pytest.raises(AssertionError):
            gi(xi, t, y, **dict(kw, cfg_scale=scale + 1))
        with pytest.raises(AssertionError):
            gi(xi, t, y, **dict(kw, cfg_interval=(0.0, 1.0)))
        with pytest.raises(AssertionError):
            gi(xi, t, y, **dict(kw, additional_model_forward=m.forward))
        with pytest.raises(AssertionError):
            gi(xi[:2], t[:2], y[:2], **kw)
        with pytest.raises(ValueError):
            fast.GraphedInferenceAutoguidance(m, x[:3], t[:3], y[:3], **kw)


def test_sample_pipeline_autoguidance_graphed_equals_ungraphed(ag_models):
    """`SamplePipeline(guidance="autoguidance")`, 4 Euler-Maruyama steps whose times cross into the interval: the graphed pipeline's latents equal the un-graphed
    one's, n samples come back, and the guide matters (the latents differ from the unguided pipeline's)."""
    from dmvae_amd.models import lightningdit_fast as fast
    from dmvae_amd.sample import SamplePipeline
    g, m, guide = ag_models
    z, y = g.t("x")[:3].to(DEV), torch.tensor([3, 10, 7], device=DEV)
    kw = dict(num_sampling_steps=4, latent_mean=0.0685, latent_scale=0.1763)
    outs = []
    for use_graph in (True, False):
        pipe = SamplePipeline(m, None, use_graph=use_graph, guidance="autoguidance", guide_model=guide, cfg_scale=2.0, cfg_interval=(0.3, 1.0), **kw)
        torch.manual_seed(77)
        outs.append(pipe.latents(z, y))
        assert isinstance(pipe._graphed, fast.GraphedInferenceAutoguidance) == use_graph
    assert outs[0].shape == (3, 64, 8) and torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    torch.manual_seed(77)
    plain = SamplePipeline(m, None, use_graph=False, **kw).latents(z, y)
    assert not torch.equal(outs[0], plain)
