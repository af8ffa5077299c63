"""The Linear, GVP and VP paths with noise-, score- and velocity-predicting models on the sampler's HIP kernels, on the MI355X (-m gpu): every `_m` entry point of csrc/sampler.hip and `dmvae_model_velocity`
bit-exact against the reference's graph written out op by op on the CPU from the same inputs (tests/transport_paths_spec.py), `sample_sde` on the small HIP
LightningDiT replayed step by step on the CPU from the model outputs the kernel route saw, and the ODE routes' drift kernel inside the fixed-grid loop and dopri5.

No tolerance: every operation is an IEEE f32 (or bf16-rounded) one, nothing is contracted, and the host supplies every scalar, formed the way the reference's
broadcast graph forms it (`transport.model_terms`, `sde._coeffs`).  `_same` of tests/test_gpu_sampler_methods.py compares NaN places.  The shapes are that
file's: scalar tail only, quads and a tail, the same through a view whose pointers forbid quads, and one past what the grid cap covers in one sweep.
The end-to-end checks replay instead of comparing with the device composition: a replay feeds the CPU graph the very model outputs the kernels consumed, so
it holds at every step whatever the device's own transcendental functions round to."""
import functools

import numpy as np
import pytest
import torch

import transport_paths_spec as S
from conftest import load_golden
from test_gpu_sampler_methods import BF, DEV, DT, FORMS, SHAPES, _dev, _inputs, _same
from test_oracle_sampler import small_dit
from test_transport_paths_cpu import PAIRS, _kw, _transport, all_paths, fixture

pytestmark = pytest.mark.gpu
KINDS = [S.NOISE, S.SCORE]
PATHS = pytest.mark.parametrize("path", [S.LINEAR, S.GVP, S.VP])
TIMES = [1e-3, 0.5139, 0.96]
DTYPES = pytest.mark.parametrize("mdtype", [torch.float32, BF], ids=["f32", "bf16"])


def _mt(kind):
    from dmvae_amd.transport import ModelType
    return {S.NOISE: ModelType.NOISE, S.SCORE: ModelType.SCORE}[kind]


def _plan(path):
    from dmvae_amd import transport as T
    return {S.LINEAR: T.ICPlan, S.GVP: T.GVPCPlan, S.VP: T.VPCPlan}[path]()


def _terms(kind, t, path=S.LINEAR):
    from dmvae_amd.transport import model_terms
    return model_terms(_plan(path), _mt(kind), t.view(1, 1))


def _scalars(t, form, norm, path=S.LINEAR):
    """(rar, var, diff, sqrt(2 diff)) at the 0-d f32 time t, from `transport.sde._coeffs` itself."""
    from dmvae_amd.transport import sde
    return sde(None, None, t0=0.0, t1=1.0, num_steps=2, sampler_type="Euler", fused=(_plan(path), form, norm))._coeffs(t)


@DTYPES
@pytest.mark.parametrize("tval", TIMES)
@pytest.mark.parametrize("kind", KINDS)
@PATHS
def test_model_velocity_kernel_bit_exact(path, kind, tval, mdtype):
    from dmvae_amd import ops
    t = torch.tensor(tval, dtype=torch.float32)
    terms = _terms(kind, t, path)
    for shape, off in SHAPES:
        x, _, m, _ = _inputs(shape)
        m = m.to(mdtype)
        want = S.velocity(kind, m, x, torch.ones(shape[0]) * t, path)
        assert want.dtype == torch.float32
        assert _same(ops.model_velocity(_dev(x, off), _dev(m, off), terms), want), (shape, off)
        out = _dev(torch.zeros(shape), off)
        assert ops.model_velocity(_dev(x, off), _dev(m, off), terms, out=out) is out and _same(out, want), (shape, off, "out")


@DTYPES
@pytest.mark.parametrize("tval", TIMES)
@pytest.mark.parametrize("form,norm", FORMS)
@pytest.mark.parametrize("kind", KINDS)
@PATHS
def test_euler_and_heun_step_kernels_bit_exact(path, kind, form, norm, tval, mdtype):
    """ops.sde_euler_step_m (with noise: the step; without: the "Mean" last step), sde_heun_predict_m and sde_heun_correct_m == the reference's steps
    (integrators.py:27-48 over transport.py:171-181, 253-256) on the CPU; each kernel is fed the reference's own intermediate values."""
    from dmvae_amd import ops
    t = torch.tensor(tval, dtype=torch.float32)
    rar, var, diff, sq2d = _scalars(t, form, norm, path)
    rar2, var2, diff2, _ = _scalars(t + DT, form, norm, path)
    terms, terms2 = _terms(kind, t, path), _terms(kind, t + DT, path)
    for shape, off in SHAPES:
        x, w, m1, m2 = _inputs(shape)
        m1, m2 = m1.to(mdtype), m2.to(mdtype)
        t_cur = torch.ones(shape[0]) * t
        d = lambda a: _dev(a, off)
        x_new, mean = S.euler_step(kind, x, m1, w, t_cur, DT, form, norm, path)
        got_x, got_mean = ops.sde_euler_step_m(d(x), d(m1), terms, d(w), rar, var, diff, float(DT), sq2d, float(torch.sqrt(DT)), need_mean=True)
        assert _same(got_x, x_new) and _same(got_mean, mean), (shape, off, "euler")
        last, _ = S.euler_step(kind, x, m1, None, t_cur, 0.04, form, norm, path)
        assert _same(ops.sde_euler_step_m(d(x), d(m1), terms, None, rar, var, diff, 0.04, 0.0, 0.0)[0], last), (shape, off, "mean")
        xhat = S.heun_perturb(x, w, t_cur, DT, form, norm, path)
        k1, xp = S.heun_predict(kind, xhat, m1, t_cur, DT, form, norm, path)
        want = S.heun_correct(kind, xhat, xp, k1, m2, t_cur + DT, DT, form, norm, path)
        got_k1, got_xp = ops.sde_heun_predict_m(d(xhat), d(m1), terms, rar, var, diff, float(DT))
        assert _same(got_k1, k1) and _same(got_xp, xp), (shape, off, "predict")
        assert _same(ops.sde_heun_correct_m(d(xhat), d(xp), d(k1), d(m2), terms2, rar2, var2, diff2, float(0.5 * DT)), want), (shape, off, "correct")


@DTYPES
@pytest.mark.parametrize("tval", TIMES)
@pytest.mark.parametrize("mode,h", [("Tweedie", 0.04), ("Euler", 0.04), ("Euler", 0.1)])
@pytest.mark.parametrize("kind", KINDS)
@PATHS
def test_last_step_kernel_bit_exact(path, kind, mode, h, tval, mdtype):
    """ops.sde_last_step_m == the reference's "Tweedie" and "Euler" last steps (transport.py:279-288) on the CPU with the model's output in the type the model
    returns it in.  Tweedie takes the model's own score, not the one converted from the velocity."""
    from dmvae_amd import ops
    t1 = torch.tensor(tval, dtype=torch.float32)
    terms, ps = _terms(kind, t1, path), _plan(path)
    for shape, off in SHAPES:
        x, _, m, _ = _inputs(shape)
        m = m.to(mdtype)
        t = torch.ones(shape[0]) * t1
        if mode == "Tweedie":
            want = S.tweedie(kind, x, m, t, path)
            a, sigma = ps.compute_alpha_t(t1.view(1, 1))[0], ps.compute_sigma_t(t1.view(1, 1))[0]      # as `Sampler._last_step` forms them
            got = ops.sde_last_step_m(_dev(x, off), _dev(m, off), terms, ops.LAST_STEP_TWEEDIE, a=float(a), c=float((sigma ** 2) / a))
        else:
            want = S.euler_last(kind, x, m, t, h, path)
            got = ops.sde_last_step_m(_dev(x, off), _dev(m, off), terms, ops.LAST_STEP_EULER, h=h)
        assert want.dtype == torch.float32 and _same(got, want), (shape, off)


@DTYPES
@pytest.mark.parametrize("tval", TIMES)
@pytest.mark.parametrize("form,norm", FORMS)
@pytest.mark.parametrize("path", [S.GVP, S.VP])
def test_velocity_model_on_gvp_and_vp_runs_on_the_existing_kernels_bit_exact(path, form, norm, tval, mdtype):
    """A velocity model needs no new kernel on a curved path: `ops.sde_euler_step`, `sde_heun_perturb` / `_predict` / `_correct` and `sde_last_step` with the new
    plans' scalars (from `sde._coeffs`, on the CPU) == the reference's graph for that path."""
    from dmvae_amd import ops
    V = S.VELOCITY
    t = torch.tensor(tval, dtype=torch.float32)
    rar, var, diff, sq2d = _scalars(t, form, norm, path)
    rar2, var2, diff2, _ = _scalars(t + DT, form, norm, path)
    ps, te = _plan(path), t.view(1, 1)
    for shape, off in SHAPES:
        x, w, v1, v2 = _inputs(shape)
        v1, v2 = v1.to(mdtype), v2.to(mdtype)
        t_cur = torch.ones(shape[0]) * t
        d = lambda a: _dev(a, off)
        if x.numel() % 4 == 0 and not off:                         # this older kernel takes whole aligned quads only; the sampler composes the step otherwise
            x_new, mean = S.euler_step(V, x, v1, w, t_cur, DT, form, norm, path)
            got_x, got_mean = ops.sde_euler_step(d(x), d(v1), d(w), rar, var, diff, float(DT), sq2d, float(torch.sqrt(DT)), need_mean=True)
            assert _same(got_x, x_new) and _same(got_mean, mean), (shape, off, "euler")
        xhat = S.heun_perturb(x, w, t_cur, DT, form, norm, path)
        k1, xp = S.heun_predict(V, xhat, v1, t_cur, DT, form, norm, path)
        want = S.heun_correct(V, xhat, xp, k1, v2, t_cur + DT, DT, form, norm, path)
        assert _same(ops.sde_heun_perturb(d(x), d(w), sq2d, float(torch.sqrt(DT))), xhat), (shape, off, "perturb")
        got_k1, got_xp = ops.sde_heun_predict(d(xhat), d(v1), rar, var, diff, float(DT))
        assert _same(got_k1, k1) and _same(got_xp, xp), (shape, off, "predict")
        assert _same(ops.sde_heun_correct(d(xhat), d(xp), d(k1), d(v2), rar2, var2, diff2, float(0.5 * DT)), want), (shape, off, "correct")
        a = ps.compute_alpha_t(te)[0]
        r1, vr1 = ps._score_coeffs(te)
        got = ops.sde_last_step(d(x), d(v1), ops.LAST_STEP_TWEEDIE, a=float(a), c=float((ps.compute_sigma_t(te)[0] ** 2) / a), rar=float(r1), var=float(vr1))
        assert _same(got, S.tweedie(V, x, v1, t_cur, path)), (shape, off, "tweedie")


def test_tweedie_of_a_bf16_score_model_rounds_the_product_to_bf16():
    """The promotion trap: (sigma^2 / alpha) is a 0-d f32 tensor and the first factor, so its product with a bf16 score is a bf16 one -- the factor is cast to
    bf16, the f32 product rounded to bf16 -- before it meets x / alpha.  The reference's graph does round there (its result differs from the one an f32 product
    gives and from the one an unrounded factor gives), the kernel follows it, and a bf16 NOISE output does not round (m / -sigma is f32)."""
    from dmvae_amd import ops
    t1 = torch.tensor(0.5139, dtype=torch.float32)
    x, _, m, _ = _inputs((5, 8, 6, 6))
    mb, t = m.to(BF), torch.ones(5) * t1
    a, c = float(t1), float(((1 - t1) ** 2) / t1)
    want = S.tweedie(S.SCORE, x, mb, t)
    f32_product = x / t1 + ((1 - t1) ** 2) / t1 * mb.float()
    cf = ((1 - t1) ** 2) / t1
    assert not torch.equal(want, f32_product) and not torch.equal(want, x / t1 + (cf * mb.float()).to(BF))
    assert torch.equal(want, x / t1 + (cf.to(BF).float() * mb.float()).to(BF))
    got = ops.sde_last_step_m(x.to(DEV), mb.to(DEV), _terms(S.SCORE, t1), ops.LAST_STEP_TWEEDIE, a=a, c=c)
    assert _same(got, want)
    got_n = ops.sde_last_step_m(x.to(DEV), mb.to(DEV), _terms(S.NOISE, t1), ops.LAST_STEP_TWEEDIE, a=a, c=c)
    assert _same(got_n, S.tweedie(S.NOISE, x, mb, t)) and _same(got_n, S.tweedie(S.NOISE, x, mb.float(), t))


def test_new_ops_validate_inputs():
    from dmvae_amd import ops
    x = torch.zeros(2, 3, 2, 2, device=DEV)
    tm = (ops.MODEL_NOISE, 1.0, 1.0, -0.5)
    with pytest.raises(ValueError):
        ops.model_velocity(x, x[:1], tm)                                              # shapes differ
    with pytest.raises(TypeError):
        ops.model_velocity(x.to(BF), x, tm)                                           # the state is f32
    with pytest.raises(TypeError):
        ops.model_velocity(x, x.double(), tm)                                         # m: bf16 or f32
    with pytest.raises(ValueError):
        ops.model_velocity(x, x, tm, out=x[:1])                                       # out of x's shape
    with pytest.raises(TypeError):
        ops.model_velocity(x, x, tm, out=x.to(BF))                                    # out is f32
    with pytest.raises(ValueError):
        ops.sde_euler_step_m(x, x, tm, x[:1], 0.5, 0.5, 0.5, 0.1, 1.0, 1.0)           # w of another shape
    with pytest.raises(TypeError):
        ops.sde_euler_step_m(x.to(BF), x, tm, None, 0.5, 0.5, 0.5, 0.1, 1.0, 1.0)
    with pytest.raises(ValueError):
        ops.sde_euler_step_m(x, x.transpose(2, 3), tm, None, 0.5, 0.5, 0.5, 0.1, 1.0, 1.0)      # not contiguous
    with pytest.raises(TypeError):
        ops.sde_heun_predict_m(x.to(BF), x, tm, 0.5, 0.5, 0.5, 0.1)
    with pytest.raises(TypeError):
        ops.sde_heun_correct_m(x, x, x, x.double(), tm, 0.5, 0.5, 0.5, 0.05)
    with pytest.raises(ValueError):
        ops.sde_heun_correct_m(x, x[:1], x, x, tm, 0.5, 0.5, 0.5, 0.05)
    with pytest.raises(ValueError):
        ops.sde_last_step_m(x, x.transpose(2, 3), tm, ops.LAST_STEP_EULER, h=0.04)
    with pytest.raises(ValueError):
        ops.sde_last_step_m(x, x, tm, 2)
    with pytest.raises(ValueError):
        ops.sde_last_step_m(x, x, (0, 1.0, 1.0, 1.0), ops.LAST_STEP_EULER, h=0.04)    # kind: NOISE or SCORE


class _Recorder:
    """Wraps a model: every evaluation's (x_in, t, m_out) is kept as CPU copies, in order."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, x, t, **kw):
        m = self.fn(x, t, **kw)
        self.calls.append((x.detach().cpu().clone(), t.detach().float().cpu().clone(), m.detach().cpu().clone()))
        return m


@functools.lru_cache(maxsize=None)
def _dit(seed):
    return small_dit(seed).to(DEV).requires_grad_(False)


@pytest.mark.parametrize("tag", ["euler", "heun"])
@pytest.mark.parametrize("path,kind", PAIRS)
def test_sample_sde_on_the_kernels_replays_bit_for_bit(path, kind, tag):
    """`sample_sde` of both captured settings (Euler / sigma / "Mean"; Heun / linear 0.7 / "Tweedie") with the small LightningDiT on the HIP kernels under
    autocast(bf16), its output read as the noise / the score: every state the kernel route returns equals the CPU spec's step from the recorded model inputs and
    outputs, every model input equals the spec's state before it, and every time vector holds the host's grid value.  The composed route
    (`FUSED_STATE_UPDATE = False`) returns finite states of the same shapes."""
    from dmvae_amd import transport as T
    g = fixture(path, kind)
    kw = _kw(g, tag)
    form, norm, lss, steps = kw["diffusion_form"], kw["diffusion_norm"], kw["last_step_size"], kw["num_steps"]
    m = _dit(int(g["dit_seed"]))
    z, y = g.t("z"), torch.from_numpy(np.asarray(g["y"]))
    rec = _Recorder(m.forward)
    with all_paths():
        tr = _transport(g)
    fn = T.Sampler(tr).sample_sde(**kw)
    t_start = tr.check_interval(tr.train_eps, tr.sample_eps, diffusion_form=form, sde=True, eval=True, last_step_size=lss)[0]
    torch.manual_seed(int(g["sde_seed"]))
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        xs = [s.cpu() for s in fn(z.to(DEV), rec, y=y.to(DEV))]
    assert len(xs) == steps and all(s.dtype == torch.float32 and s.shape == z.shape for s in xs)
    assert rec.calls[0][2].dtype == BF                               # the model does answer in bf16: the widening sites are exercised
    # replay
    ts = torch.linspace(t_start, 1 - lss, steps)      # the interval's start: tests/test_transport_paths_cpu.py holds `check_interval` to the reference's table
    dt = ts[1] - ts[0]
    torch.manual_seed(int(g["sde_seed"]))
    x, calls = z, iter(rec.calls)
    for i, ti in enumerate(ts[:-1]):
        w = torch.randn(x.size())
        tv = torch.ones(x.size(0)) * ti
        if tag == "euler":
            x_in, t_in, m1 = next(calls)
            assert torch.equal(x_in, x) and torch.equal(t_in, tv), i
            x, _ = S.euler_step(kind, x, m1, w, tv, dt, form, norm, path)
        else:
            xhat = S.heun_perturb(x, w, tv, dt, form, norm, path)
            x_in, t_in, m1 = next(calls)
            assert torch.equal(x_in, xhat) and torch.equal(t_in, tv), i
            k1, xp = S.heun_predict(kind, xhat, m1, tv, dt, form, norm, path)
            x_in, t_in, m2 = next(calls)
            assert torch.equal(x_in, xp) and torch.equal(t_in, tv + dt), i
            x = S.heun_correct(kind, xhat, xp, k1, m2, tv + dt, dt, form, norm, path)
        assert torch.equal(xs[i], x), (i, (xs[i] - x).abs().max())
    x_in, t_in, ml = next(calls)
    tv = torch.ones(x.size(0)) * (1 - lss)
    assert torch.equal(x_in, x) and torch.equal(t_in, tv)
    last = S.euler_step(kind, x, ml, None, tv, lss, form, norm, path)[0] if kw["last_step"] == "Mean" else S.tweedie(kind, x, ml, tv, path)
    assert torch.isfinite(last).all() and torch.equal(xs[-1], last)
    assert next(calls, None) is None
    # the composition still runs
    T.FUSED_STATE_UPDATE = False
    try:
        torch.manual_seed(int(g["sde_seed"]))
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            plain = fn(z.to(DEV), m.forward, y=y.to(DEV))
    finally:
        T.FUSED_STATE_UPDATE = True
    assert len(plain) == steps and all(s.shape == z.shape and torch.isfinite(s).all() for s in plain)


@pytest.mark.parametrize("method,num_steps", [("euler", 5), ("midpoint", 3), ("heun3", 3), ("rk4", 3), ("dopri5", 3)])
@pytest.mark.parametrize("kind", KINDS)
def test_ode_routes_take_the_drift_from_the_kernel(kind, method, num_steps, monkeypatch):
    """`sample_ode` with a noise / score model: the fixed-grid loop and dopri5 (`_Dopri5.f` writes into k[slot]) take the converted drift from
    `ops.model_velocity`.  A linear stub m = a x + b t + c y keeps the problem smooth.  Every launch's output equals the CPU spec at the (x, t) the model saw -- t
    there is the device's, the kernel's scalars come from the host's twin of the time arithmetic, so the two must be the same number --, the result is finite,
    and the number of model evaluations equals the composed route's."""
    from dmvae_amd import ops
    from dmvae_amd import transport as T
    seen, launches = [], []

    def stub(x, t, y):          # the labels arrive under the keyword the reference's drivers use
        seen.append((x.cpu().clone(), t.cpu().clone()))
        return 0.3 * x + 0.1 * t.view(-1, 1, 1, 1) + 0.001 * y.view(-1, 1, 1, 1)

    real = ops.model_velocity

    def recording(x, m, terms, out=None):
        r = real(x, m, terms, out=out)
        launches.append((m.cpu().clone(), r.cpu().clone(), out is not None))
        return r

    monkeypatch.setattr(ops, "model_velocity", recording)
    with all_paths():
        tr = T.create_transport("GVP", kind, None, 1e-3, 1e-3, time_dist_shift=1.0)
    fn = T.Sampler(tr).sample_ode(sampling_method=method, num_steps=num_steps, atol=1e-5, rtol=1e-3)
    x0 = (_inputs((5, 8, 6, 6))[0] * 0.01).to(DEV)
    labels = torch.arange(5, device=DEV, dtype=torch.float32)
    with torch.no_grad():
        xs = fn(x0, stub, y=labels)
    assert xs.shape == (num_steps, 5, 8, 6, 6) and xs.dtype == torch.float32 and torch.isfinite(xs).all()
    assert len(launches) == len(seen) > 0
    for (x, t), (m, out, into) in zip(seen, launches):
        assert torch.equal(out, S.velocity(kind, m, x, t, S.GVP))
        assert into == (method == "dopri5")                         # dopri5: straight into the stage slot
    nfe = len(seen)
    seen.clear()
    T.FUSED_STATE_UPDATE = False
    try:
        with torch.no_grad():
            plain = fn(x0, stub, y=labels)
    finally:
        T.FUSED_STATE_UPDATE = True
    assert len(launches) == nfe and len(seen) == nfe                # the composed route launches no conversion kernel and evaluates as often
    assert plain.shape == xs.shape and torch.isfinite(plain).all()


def test_euler_sde_on_an_odd_element_count_equals_the_composition(monkeypatch):
    """`sample_sde(sampling_method="Euler", last_step="Mean")` on a (3, 1, 5, 1) state -- 15 elements, which the Euler-Maruyama kernel used to refuse, so that the
    sampler composed such a step -- with the linear stub of the ODE check above as a velocity model: every state of the kernel route equals the composition's
    (same noise stream), and the kernel route does launch `ops.sde_euler_step` for both steps and the last one.  The composition takes sqrt(2 diffusion) with the
    device's sqrt, which is not correctly rounded on this stack (tests/test_gpu_sampler_methods.py); the "linear" form with norm 8 on the grid
    linspace(0, 1 - 0.125, 3) = 0, 0.4375, 0.875 keeps its inputs at the exact squares 16 and 9, every product on the way exact in f32."""
    from dmvae_amd import ops
    from dmvae_amd import transport as T
    calls, real = [], ops.sde_euler_step
    monkeypatch.setattr(ops, "sde_euler_step", lambda *a, **kw: calls.append(a[0].numel()) or real(*a, **kw))
    stub = lambda x, t, y: 0.3 * x + 0.1 * t.view(-1, 1, 1, 1) + 0.001 * y.view(-1, 1, 1, 1)
    fn = T.Sampler(T.create_transport("Linear", "velocity")).sample_sde(sampling_method="Euler", diffusion_form="linear", diffusion_norm=8.0, last_step="Mean",
                                                                        last_step_size=0.125, num_steps=3)
    x0, labels = _inputs((3, 1, 5, 1))[0].to(DEV), torch.arange(3, device=DEV, dtype=torch.float32)
    runs = []
    for fused in (True, False):
        T.FUSED_STATE_UPDATE = fused
        try:
            torch.manual_seed(11)
            with torch.no_grad():
                runs.append(torch.stack(fn(x0, stub, y=labels)))
        finally:
            T.FUSED_STATE_UPDATE = True
    assert calls == [15, 15, 15]                                    # the kernel route only
    assert runs[0].shape == (3, 3, 1, 5, 1) and runs[0].dtype == torch.float32 and torch.isfinite(runs[0]).all()
    assert torch.equal(runs[0], runs[1])
