"""Host mirror of the reference's `diffusion/transport` package: the Linear path with velocity prediction (the configuration its scripts run), noise /
score prediction (`--prediction noise|score`) and, behind `enable_all_paths()`, the GVP and VP paths (`--path_type GVP|VP`):
`create_transport` (__init__.py:3-64), `Transport` (transport.py:39-221), `ICPlan` / `VPCPlan` / `GVPCPlan` (path.py:18-192), `Sampler` (transport.py:223-458) and the
`sde` / `ode` integrators (integrators.py:8-118) -- same names, arguments, defaults, random-number consumption and error behaviour.

What runs where: a sampler step is one model forward (LightningDiT on the HIP kernels, models/lightningdit_fast.py) plus the state update;
the Euler-Maruyama update -- velocity -> score, drift, mean, noise injection -- is ONE kernel pass over the state (`ops.sde_euler_step`, csrc/sampler.hip)
with the reference's f32 arithmetic order, so for the same model output the trajectory is bit-identical to the PyTorch reference.  The Heun step is three
such passes around its two evaluations (`ops.sde_heun_perturb`, `sde_heun_predict`, `sde_heun_correct`) and the "Tweedie" / "Euler" last steps one
(`ops.sde_last_step`), on the same terms.  The fixed-grid ODE methods are composed from device tensor ops; every time vector of a CUDA state is filled on the
device (`_time_vector`), so no model evaluation waits for a host-to-device copy.  The reference's default ODE method, adaptive dopri5 (torchdiffeq's, restated below), runs
on the device for a CUDA f32 state: the model forwards plus three kernels of csrc/sampler.hip per step (`ops.ode_rk_combine`, `ops.ode_error_ratio`,
`ops.ode_dense_output`) and one 8-byte readback per attempted step for the step-size controller.  The likelihood sampler (`Sampler.sample_ode_likelihood`)
integrates the tuple state (x, logp) as one flat f32 buffer with torchdiffeq's mixed norm; each evaluation is one model forward, its input-VJP and one
kernel (`ops.ode_hutchinson_pack`) that writes the stage value.  The per-step noise is drawn on the CPU generator and moved to the state's
device exactly as the reference does (`th.randn(x.size()).to(x)`, integrators.py:28,38), so a seeded run consumes the same stream.

Model types: everything downstream of the model is the same once its output is a velocity.  A noise / score model adds a prologue to each model-consuming
pass (the `_m` entry points of csrc/sampler.hip): v = (-drift_mean) + drift_var * score (transport.py:171-181), its three t-only coefficients host scalars
(`model_terms`).  Host-scalar rule: every coefficient of a kernel route is formed on the CPU in f32 from the host's copy of t by the path's own methods, never
read back from the device and never formed there.  The ODE routes take the converted drift from one kernel per evaluation (`ops.model_velocity`, written
straight into dopri5's stage slot); the likelihood sampler of a noise / score model stays composed (it needs the VJP through the conversion).

Paths: the GVP and VP plans are opt-in (`enable_all_paths()`; off, `Transport` refuses them as it always did -- `run_on_mi355x.py` turns the switch on when it
runs a script, whose own `--path_type` is then the selection).  Nothing downstream of the model depends on the path beyond the t-only scalars the plans' own
methods give on the CPU, so a velocity model on GVP / VP runs on the same kernels as on the Linear path and a noise / score model on the same `_m` kernels.
Their transcendental coefficients (sin / cos / tan, exp / sqrt of t) are exactly why the host-scalar rule holds: the device's are not the CPU's.

Not built: dopri5 and tuple states
on CPU or non-f32 states and the other adaptive ODE solvers unless `torchdiffeq` (an unpinned third-party dependency) is importable."""
from __future__ import annotations

import enum
import os

import numpy as np
import torch as th

from . import ops

FUSED_STATE_UPDATE = True      # False composes the Euler-Maruyama / Heun / last-step / dopri5 updates from tensor ops (tests/test_gpu_sampler*.py, test_gpu_ode_dopri5.py compare)


class ModelType(enum.Enum):
    NOISE = enum.auto()
    SCORE = enum.auto()
    VELOCITY = enum.auto()


class PathType(enum.Enum):
    LINEAR = enum.auto()
    GVP = enum.auto()
    VP = enum.auto()


class WeightType(enum.Enum):
    NONE = enum.auto()
    VELOCITY = enum.auto()
    LIKELIHOOD = enum.auto()


def expand_t_like_x(t, x):
    """path.py:5-13."""
    return t.view(t.size(0), *([1] * (x.dim() - 1)))


def mean_flat(x):
    """utils.py:12-16."""
    return th.mean(x, dim=list(range(1, x.dim())))


class ICPlan:
    """Linear coupling plan x_t = t x1 + (1 - t) x0 (path.py:18-136).  Every method works on tensors of any device, like the reference's."""

    def __init__(self, sigma=0.0):
        self.sigma = sigma

    def compute_alpha_t(self, t):
        return t, 1

    def compute_sigma_t(self, t):
        return 1 - t, -1

    def compute_d_alpha_alpha_ratio_t(self, t):
        return 1 / t

    def compute_drift(self, x, t):
        t = expand_t_like_x(t, x)
        ratio = self.compute_d_alpha_alpha_ratio_t(t)
        sigma_t, d_sigma_t = self.compute_sigma_t(t)
        return -(ratio * x), ratio * (sigma_t ** 2) - sigma_t * d_sigma_t

    def compute_diffusion(self, x, t, form="constant", norm=1.0):
        t = expand_t_like_x(t, x)
        if form == "constant":
            return norm
        if form == "SBDM":
            return norm * self.compute_drift(x, t)[1]
        if form == "sigma":
            return norm * self.compute_sigma_t(t)[0]
        if form == "linear":
            return norm * (1 - t)
        if form == "decreasing":
            return 0.25 * (norm * th.cos(np.pi * t) + 1) ** 2
        if form == "inccreasing-decreasing":            # the reference's spelling (path.py:59)
            return norm * th.sin(np.pi * t) ** 2
        raise NotImplementedError(f"Diffusion form {form} not implemented")

    def _score_coeffs(self, t):
        """(reverse_alpha_ratio, var) of get_score_from_velocity, in the reference's operation order (path.py:82-88)."""
        alpha_t, d_alpha_t = self.compute_alpha_t(t)
        sigma_t, d_sigma_t = self.compute_sigma_t(t)
        rar = alpha_t / d_alpha_t
        return rar, sigma_t ** 2 - rar * d_sigma_t * sigma_t

    def get_score_from_velocity(self, velocity, x, t):
        rar, var = self._score_coeffs(expand_t_like_x(t, x))
        return (rar * velocity - x) / var

    def get_noise_from_velocity(self, velocity, x, t):
        t = expand_t_like_x(t, x)
        alpha_t, d_alpha_t = self.compute_alpha_t(t)
        sigma_t, d_sigma_t = self.compute_sigma_t(t)
        rar = alpha_t / d_alpha_t
        return (rar * velocity - x) / (rar * d_sigma_t - sigma_t)

    def get_velocity_from_score(self, score, x, t):
        drift, var = self.compute_drift(x, expand_t_like_x(t, x))
        return var * score - drift

    def compute_mu_t(self, t, x0, x1):
        t = expand_t_like_x(t, x1)
        return self.compute_alpha_t(t)[0] * x1 + self.compute_sigma_t(t)[0] * x0

    def compute_xt(self, t, x0, x1):
        return self.compute_mu_t(t, x0, x1)

    def compute_ut(self, t, x0, x1, xt):
        t = expand_t_like_x(t, x1)
        return self.compute_alpha_t(t)[1] * x1 + self.compute_sigma_t(t)[1] * x0

    def plan(self, t, x0, x1):
        xt = self.compute_xt(t, x0, x1)
        return t, xt, self.compute_ut(t, x0, x1, xt)


class VPCPlan(ICPlan):
    """Variance-preserving path (path.py:139-171): alpha_t = exp(log_mean_coeff(t)), sigma_t = sqrt(1 - alpha_t^2), with its own `compute_drift`."""

    def __init__(self, sigma_min=0.1, sigma_max=20.0):
        self.sigma_min = sigma_min
        self.sigma_max = sigma_max

    def log_mean_coeff(self, t):
        return -0.25 * ((1 - t) ** 2) * (self.sigma_max - self.sigma_min) - 0.5 * (1 - t) * self.sigma_min

    def d_log_mean_coeff(self, t):
        return 0.5 * (1 - t) * (self.sigma_max - self.sigma_min) + 0.5 * self.sigma_min

    def compute_alpha_t(self, t):
        alpha_t = th.exp(self.log_mean_coeff(t))
        return alpha_t, alpha_t * self.d_log_mean_coeff(t)

    def compute_sigma_t(self, t):
        p_sigma_t = 2 * self.log_mean_coeff(t)
        sigma_t = th.sqrt(1 - th.exp(p_sigma_t))
        return sigma_t, th.exp(p_sigma_t) * (2 * self.d_log_mean_coeff(t)) / (-2 * sigma_t)

    def compute_d_alpha_alpha_ratio_t(self, t):
        return self.d_log_mean_coeff(t)

    def compute_drift(self, x, t):
        t = expand_t_like_x(t, x)
        beta_t = self.sigma_min + (1 - t) * (self.sigma_max - self.sigma_min)
        return -0.5 * beta_t * x, beta_t / 2


class GVPCPlan(ICPlan):
    """Trigonometric (generalised VP) path (path.py:174-192): alpha_t = sin(pi t / 2), sigma_t = cos(pi t / 2)."""

    def compute_alpha_t(self, t):
        return th.sin(t * np.pi / 2), np.pi / 2 * th.cos(t * np.pi / 2)

    def compute_sigma_t(self, t):
        return th.cos(t * np.pi / 2), -np.pi / 2 * th.sin(t * np.pi / 2)

    def compute_d_alpha_alpha_ratio_t(self, t):
        return np.pi / (2 * th.tan(t * np.pi / 2))


_ALL_PATHS = False


def enable_all_paths(on: bool = True) -> bool:
    """Let `Transport` build the GVP and VP plans (off by default: only the Linear path, as the reference's scripts select it) -> the previous setting."""
    global _ALL_PATHS
    prev, _ALL_PATHS = _ALL_PATHS, bool(on)
    return prev


def model_terms(ps, model_type, te):
    """The prologue scalars (kind, c0, dv, nsig) of a noise / score model at the CPU f32 time te [1, 1], from the path's own methods on the CPU:
    v = c0 * x + dv * (m / nsig) (NOISE) or c0 * x + dv * m (SCORE) is the reference's (-drift_mean) + drift_var * score (transport.py:171-181).  drift_mean is
    -(ratio * x) (Linear, GVP) or (-0.5 * beta_t) * x (VP), so at x = 1 its negation is c0 itself (a product with 1 and a negation are exact)."""
    assert not te.is_cuda and te.dtype == th.float32
    drift_mean, dv = ps.compute_drift(th.ones(1, 1), te.view(1))
    nsig = -ps.compute_sigma_t(te)[0]
    kind = {ModelType.NOISE: ops.MODEL_NOISE, ModelType.SCORE: ops.MODEL_SCORE}[model_type]
    return kind, float(-drift_mean), float(dv), float(nsig)


_RAND_RING = {}


def cpu_rand_like_batch(x1):
    """`th.rand((B,)).to(x1)` (transport.py:110-111): the batch's times drawn on the CPU generator, like the reference, and handed to x1's device WITHOUT stalling
    the launch queue: the draw lands in one of four pinned staging buffers and is copied with non_blocking (a pageable copy waits for the stream -- once per
    training step the host then stood still until the device had caught up, and every kernel after it was launched with the device on its heels:
    tools/probes/host_ahead.py; the sampler's `_noise` does the same for its per-step noise)."""
    n = x1.shape[0]
    if not x1.is_cuda:
        return th.rand((n,))
    key = (n, x1.device)
    ring = _RAND_RING.get(key)
    if ring is None:
        ring = _RAND_RING[key] = [[[th.empty((n,), dtype=th.float32).pin_memory(), None] for _ in range(4)], 0]
    slot = ring[0][ring[1]]
    ring[1] = (ring[1] + 1) % len(ring[0])
    if slot[1] is not None:
        slot[1].synchronize()                        # the copy that last used this buffer (four draws ago) has finished
    th.rand((n,), out=slot[0])
    t = slot[0].to(device=x1.device, non_blocking=True)
    slot[1] = th.cuda.Event()
    slot[1].record()
    return t                                          # f32 on x1's device: the caller casts where the reference's `.to(x1)` stands


class Transport:
    """transport.py:39-221."""

    def __init__(self, *, model_type, path_type, loss_type, train_eps, sample_eps, time_dist_shift=1.0):
        if path_type != PathType.LINEAR and not _ALL_PATHS:
            raise NotImplementedError("only the Linear path (path.ICPlan) is built by default; the reference's scripts never select GVP / VP -- "
                                      "dmvae_amd.transport.enable_all_paths() turns the GVP / VP plans on")
        self.loss_type = loss_type
        self.model_type = model_type
        self.path_sampler = {PathType.LINEAR: ICPlan, PathType.GVP: GVPCPlan, PathType.VP: VPCPlan}[path_type]()
        self.train_eps = train_eps
        self.sample_eps = sample_eps
        self.time_dist_shift = time_dist_shift

    def prior_logp(self, z):
        n = z[0].numel()
        return -n / 2.0 * np.log(2 * np.pi) - th.sum(z.flatten(1) ** 2, dim=1) / 2.0

    def check_interval(self, train_eps, sample_eps, *, diffusion_form="SBDM", sde=False, reverse=False, eval=False, last_step_size=0.0):
        """transport.py:75-102."""
        t0, t1 = 0, 1
        eps = train_eps if not eval else sample_eps
        if type(self.path_sampler) is VPCPlan:
            t1 = 1 - eps if (not sde or last_step_size == 0) else 1 - last_step_size
        elif self.model_type != ModelType.VELOCITY or sde:
            t0 = eps if (diffusion_form == "SBDM" and sde) or self.model_type != ModelType.VELOCITY else 0
            t1 = 1 - eps if (not sde or last_step_size == 0) else 1 - last_step_size
        if reverse:
            t0, t1 = 1 - t0, 1 - t1
        return t0, t1

    def sample(self, x1):
        """transport.py:105-116: x0 on x1's device generator, t on the CPU generator, then the time shift."""
        x0 = th.randn_like(x1)
        t0, t1 = self.check_interval(self.train_eps, self.sample_eps)
        t = cpu_rand_like_batch(x1) * (t1 - t0) + t0
        t = t.to(x1)
        t = 1 - self.time_dist_shift * (1 - t) / (1 + (self.time_dist_shift - 1) * (1 - t))
        return t, x0, x1

    def training_losses(self, model, x1, model_kwargs=None):
        """transport.py:119-164: flow-matching loss per sample, `terms = {"pred", "loss"}` -- the velocity MSE for every model type, as in the reference (its
        per-model-type weights are commented out, transport.py:142-162; `loss_type` is kept and unused)."""
        if model_kwargs is None:
            model_kwargs = {}
        t, x0, x1 = self.sample(x1)
        t, xt, ut = self.path_sampler.plan(t, x0, x1)
        model_output = model(xt, t, **model_kwargs)
        assert model_output.size() == xt.size()
        return t, {"pred": model_output, "loss": mean_flat((model_output - ut) ** 2)}

    def get_drift(self):
        """transport.py:167-199."""
        ps = self.path_sampler

        def score_ode(x, t, model, **kw):
            drift_mean, drift_var = ps.compute_drift(x, t)
            return -drift_mean + drift_var * model(x, t, **kw)

        def noise_ode(x, t, model, **kw):
            drift_mean, drift_var = ps.compute_drift(x, t)
            sigma_t, _ = ps.compute_sigma_t(expand_t_like_x(t, x))
            return -drift_mean + drift_var * (model(x, t, **kw) / -sigma_t)

        def velocity_ode(x, t, model, **kw):
            return model(x, t, **kw)

        fn = {ModelType.NOISE: noise_ode, ModelType.SCORE: score_ode}.get(self.model_type, velocity_ode)

        def body_fn(x, t, model, **kw):
            out = fn(x, t, model, **kw)
            assert out.shape == x.shape, "Output shape from ODE solver must match input shape"
            return out

        return body_fn

    def get_score(self):
        """transport.py:202-216."""
        ps = self.path_sampler
        if self.model_type == ModelType.NOISE:
            return lambda x, t, model, **kw: model(x, t, **kw) / -ps.compute_sigma_t(expand_t_like_x(t, x))[0]
        if self.model_type == ModelType.SCORE:
            return lambda x, t, model, **kw: model(x, t, **kw)
        if self.model_type == ModelType.VELOCITY:
            return lambda x, t, model, **kw: ps.get_score_from_velocity(model(x, t, **kw), x, t)
        raise NotImplementedError()

    def convert_score(self, score, x, t):
        return self.path_sampler.get_score_from_velocity(score, x, t)


def create_transport(path_type="Linear", prediction="velocity", loss_weight=None, train_eps=None, sample_eps=None, time_dist_shift=1.0):
    """__init__.py:3-64 (including its quirk that `sample_eps` falls back on `train_eps is None`)."""
    model_type = {"noise": ModelType.NOISE, "score": ModelType.SCORE}.get(prediction, ModelType.VELOCITY)
    loss_type = {"velocity": WeightType.VELOCITY, "likelihood": WeightType.LIKELIHOOD}.get(loss_weight, WeightType.NONE)
    path = {"Linear": PathType.LINEAR, "GVP": PathType.GVP, "VP": PathType.VP}[path_type]
    if path == PathType.VP:
        train_eps, sample_eps = (1e-5 if train_eps is None else train_eps), (1e-3 if train_eps is None else sample_eps)
    elif model_type != ModelType.VELOCITY:
        train_eps, sample_eps = (1e-3 if train_eps is None else train_eps), (1e-3 if train_eps is None else sample_eps)
    else:
        train_eps = sample_eps = 0
    return Transport(model_type=model_type, path_type=path, loss_type=loss_type, train_eps=train_eps, sample_eps=sample_eps,
                     time_dist_shift=time_dist_shift)


# ---- integrators -----------------------------------------------------------------------------------------------------------------------
def _time_vector(n, t, like=None, device=None):
    """The model's time vector `th.ones(n).to(x) * t` (integrators.py:28-29,38-39; `.to(device)` at :108): the same values and bits.  For a CUDA state it is
    filled on the device -- the reference's pageable host-to-device copy of the ones waits for the stream, once per model evaluation."""
    device, dtype = (like.device, like.dtype) if like is not None else (th.device(device), th.float32)
    if device.type != "cuda":
        return (th.ones(n).to(like) if like is not None else th.ones(n).to(device)) * t
    if th.is_tensor(t) and t.is_cuda:                       # the fixed-grid ODE loop's grid lives on the device: no host read of t either
        return th.full((n,), 1.0, device=device, dtype=dtype) * t
    return th.full((n,), float(t), device=device, dtype=dtype)


class sde:
    """integrators.py:8-77.  `sampler_type` "Euler" (Euler-Maruyama) or "Heun".

    With `fused` (set by `Sampler.sample_sde`) a step calls the model and does the whole
    update on csrc/sampler.hip -- Euler-Maruyama in `ops.sde_euler_step`, Heun in `ops.sde_heun_perturb` / `sde_heun_predict` / `sde_heun_correct` around its
    two evaluations; for a noise / score model with `terms=`, which converts the model's output to the velocity first (`model_terms`) --; otherwise it
    evaluates the caller's `drift` / `diffusion` callables like the reference."""

    def __init__(self, drift, diffusion, *, t0, t1, num_steps, sampler_type, fused=None):
        assert t0 < t1, "SDE sampler has to be in forward time"
        self.num_timesteps = num_steps
        self.t = th.linspace(t0, t1, num_steps)
        self.dt = self.t[1] - self.t[0]
        self.drift = drift
        self.diffusion = diffusion
        self.sampler_type = sampler_type
        self.fused = fused                     # (path_sampler, diffusion_form, diffusion_norm[, model_type = VELOCITY]) or None

    def _noise(self, x):
        """`th.randn(x.size()).to(x)` (integrators.py:28,38): drawn on the CPU generator like the reference.  For a device state the draw lands in one of
        four pinned staging buffers and is copied without blocking the host, so the next kernels are queued while the previous step still runs (a
        pageable copy stalls the launch queue once per step: 1.4 ms of 13 at sample_50k's batch)."""
        if not x.is_cuda:
            return th.randn(x.size()).to(x)
        ring = getattr(self, "_ring", None)
        if ring is None or ring[0][0].shape != x.shape:
            ring = self._ring = [[th.empty(x.size(), dtype=th.float32).pin_memory(), None] for _ in range(4)]
            self._ring_i = 0
        slot = ring[self._ring_i]
        self._ring_i = (self._ring_i + 1) % len(ring)
        if slot[1] is not None:
            slot[1].synchronize()                        # the copy that last used this buffer (four steps ago) has finished
        th.randn(x.size(), out=slot[0])
        w = slot[0].to(device=x.device, non_blocking=True)
        slot[1] = th.cuda.Event()
        slot[1].record()
        return w if w.dtype == x.dtype else w.to(x.dtype)

    def _coeffs(self, ti):
        """The scalars of one fused step, computed in f32 the way the reference's broadcast graph computes them."""
        ps, form, norm = self.fused[:3]
        te = ti.view(1, 1)
        rar, var = ps._score_coeffs(te)
        diff = ps.compute_diffusion(te, te.view(1), form=form, norm=norm)
        diff = diff if th.is_tensor(diff) else th.tensor(float(diff), dtype=th.float32)
        return float(rar), float(var), float(diff), float(th.sqrt(2 * diff))

    def _terms(self, ti):
        """The prologue scalars of a noise / score model at the CPU f32 time ti (`model_terms`); None for a velocity model."""
        mt = self.fused[3] if len(self.fused) > 3 else ModelType.VELOCITY
        return None if mt == ModelType.VELOCITY else model_terms(self.fused[0], mt, ti.view(1, 1))

    def _fused_ok(self, x):
        return FUSED_STATE_UPDATE and self.fused is not None and x.is_cuda and x.dtype == th.float32

    def _euler_maruyama_step(self, x, mean_x, t, model, **model_kwargs):
        w_cur = self._noise(x)
        if self._fused_ok(x):
            terms = self._terms(t)
            m = model(x, _time_vector(x.size(0), t, x), **model_kwargs)
            assert m.shape == x.shape, "Output shape from ODE solver must match input shape"
            rar, var, diff, sq2d = self._coeffs(t)
            return ops.sde_euler_step(x.contiguous(), m.contiguous(), w_cur, rar, var, diff, float(self.dt), sq2d, float(th.sqrt(self.dt)),
                                      need_mean=True, terms=terms)
        # composed from tensor ops: the noise scaled by sqrt(dt) and by sqrt(2 diffusion), added to the deterministic part of the step
        h = self.dt
        tv = _time_vector(x.size(0), t, x)
        noise = th.sqrt(h) * w_cur
        f = self.drift(x, tv, model, **model_kwargs)
        g = th.sqrt(2 * self.diffusion(x, tv))
        mean_x = f * h + x
        return g * noise + mean_x, mean_x

    def _heun_step(self, x, _, t, model, **model_kwargs):
        w_cur = self._noise(x)
        if self._fused_ok(x):
            # three passes around the two evaluations; the corrector's coefficients and its time vector at the f32 sum t + dt, as `t_cur + self.dt` holds it
            n, t2 = x.size(0), t + self.dt
            rar, var, diff, sq2d = self._coeffs(t)
            rar2, var2, diff2, _ = self._coeffs(t2)
            terms, terms2 = self._terms(t), self._terms(t2)
            xhat = ops.sde_heun_perturb(x.contiguous(), w_cur, sq2d, float(th.sqrt(self.dt)))
            v1 = model(xhat, _time_vector(n, t, x), **model_kwargs)
            assert v1.shape == x.shape, "Output shape from ODE solver must match input shape"
            # v1 is consumed here: a graphed model reuses its output buffer
            k1, xp = ops.sde_heun_predict(xhat, v1.contiguous(), rar, var, diff, float(self.dt), terms=terms)
            v2 = model(xp, _time_vector(n, t2, x), **model_kwargs)
            assert v2.shape == x.shape, "Output shape from ODE solver must match input shape"
            return ops.sde_heun_correct(xhat, xp, k1, v2.contiguous(), rar2, var2, diff2, float(0.5 * self.dt), terms=terms2), xhat
        noise = th.sqrt(self.dt) * w_cur
        t_cur = _time_vector(x.size(0), t, x)
        diffusion = self.diffusion(x, t_cur)
        xhat = x + th.sqrt(2 * diffusion) * noise
        k1 = self.drift(xhat, t_cur, model, **model_kwargs)
        xp = xhat + self.dt * k1
        k2 = self.drift(xp, t_cur + self.dt, model, **model_kwargs)
        return xhat + 0.5 * self.dt * (k1 + k2), xhat

    def sample(self, init, model, **model_kwargs):
        try:
            step = {"Euler": self._euler_maruyama_step, "Heun": self._heun_step}[self.sampler_type]
        except KeyError:
            raise NotImplementedError(f"sde: sampler_type must be \"Euler\" or \"Heun\", got {self.sampler_type!r}") from None
        x, mean_x, samples = init, init, []
        for ti in self.t[:-1]:
            with th.no_grad():
                x, mean_x = step(x, mean_x, ti, model, **model_kwargs)
                samples.append(x)
        return samples


_FIXED_GRID = ("euler", "midpoint", "heun3", "rk4")

# ---- dopri5: torchdiffeq 0.2.x's RKAdaptiveStepsizeODESolver with the Dormand-Prince-Shampine tableau (integrators.py:79-118 hands it the drift).
# Unpinned (torchdiffeq is not a dependency); tests/dopri5_spec.py restates the method in float64 with exact fractions.  The tableau is written as
# torchdiffeq writes it (float64 quotients, cast to the state's dtype).
DOPRI5_ALPHA = (1 / 5, 3 / 10, 4 / 5, 8 / 9, 1., 1.)
DOPRI5_BETA = ((1 / 5,),
               (3 / 40, 9 / 40),
               (44 / 45, -56 / 15, 32 / 9),
               (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
               (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
               (35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84))
DOPRI5_C_ERROR = (35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 - -12231 / 42400, 11 / 84 - 649 / 6300,
                  -1. / 60.)
DOPRI5_C_MID = (6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2, 187940372067 / 1594534317056 / 2,
                -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2)


def dopri5_initial_h0(d0: float, d1: float) -> float:
    """_select_initial_step's first guess from d0 = rms(y0 / scale), d1 = rms(f0 / scale)."""
    return 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1


def dopri5_initial_dt(h0: float, d1: float, d2: float, order: int = 4) -> float:
    """_select_initial_step's result from h0, d1 and d2 = rms((f1 - f0) / scale) / h0; dopri5 passes order 5 - 1."""
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1. / (order + 1))
    return min(100 * h0, h1)


def dopri5_next_dt(dt: float, ratio: float, safety=0.9, ifactor=10.0, dfactor=0.2, order=5) -> float:
    """_optimal_step_size: the step after one with error ratio `ratio` (accepted or not).  A NaN ratio gives a NaN step, which the next step's
    underflow check turns into an error (torch.max / torch.min propagate NaN; Python's min / max would not)."""
    if ratio != ratio:
        return float("nan")
    if ratio == 0:
        return dt * ifactor
    if ratio < 1:
        dfactor = 1.0
    return dt * min(ifactor, max(safety / ratio ** (1. / order), dfactor))


def dopri5_accept(ratio: float) -> bool:
    return ratio <= 1


def dopri5_stage_times(t0: float, dt: float):
    """The six stage times of a step from t0 (float64): t0 + alpha_i dt in the state's dtype (f32), the last two at t1 = t0 + dt (float64, then f32)."""
    t, h = np.float32(t0), np.float32(dt)
    return [np.float32(t + np.float32(a) * h) for a in DOPRI5_ALPHA[:4]] + [np.float32(t0 + dt)] * 2


def dopri5_weights(coef, dt: float):
    """coef * dt in f32, as torchdiffeq's `beta_i * dt` / `dt * c_error` / `dt * mid` with the tableau cast to the state's dtype."""
    return [float(np.float32(c) * np.float32(dt)) for c in coef]


def dopri5_dense_x(t: float, t0: float, t1: float) -> float:
    """_interp_evaluate's x, formed in float64 and cast to the state's dtype."""
    return float(np.float32((t - t0) / (t1 - t0)))


def dopri5_pending_outputs(ts, i: int, t1: float):
    """Grid bookkeeping: the indices of the output times from i on that the step ending at t1 covers (torchdiffeq steps while t_i > t1)."""
    j = i
    while j < len(ts) and ts[j] <= t1:
        j += 1
    return range(i, j)


def _rms(v):
    return v.abs().pow(2).mean().sqrt()


class _Dopri5:
    """The solver on a CUDA f32 state.  fused: the combine / error-ratio / dense-output kernels of csrc/sampler.hip and one 8-byte readback per
    attempted step; else the same algorithm composed from tensor ops (what the kernels are tested against).  round_bf16: the three weighted sums
    in the bf16 form torchdiffeq's k.matmul takes under autocast(bf16).
    A tuple state (the likelihood sampler's (x, logp)) is ONE flat f32 buffer, as torchdiffeq's _TupleFunc holds it: `parts` are its [start, stop) ranges,
    `batch` the samples the model's t vector needs, and `fn_into(t, y, out)` writes the drift of the flat state into the flat stage slot.  Norms are then
    torchdiffeq's _mixed_norm -- the max over the parts of each part's RMS -- in the initial step and in the error ratio (one error-ratio launch pair per part,
    8 bytes read back per part and attempted step); the combine and dense-output kernels run on the whole buffer."""

    def __init__(self, fn, y0, *, atol, rtol, fused, round_bf16, parts=None, batch=None, fn_into=None, fn_into_t=None):
        self.fn, self.atol, self.rtol, self.fused, self.amp = fn, float(atol), float(rtol), fused, round_bf16
        self.parts, self.fn_into, self.fn_into_t = parts, fn_into, fn_into_t      # fn_into_t(t32, tv, y, out): fn_into that also gets the host's f32 time
        self.batch = y0.size(0) if batch is None else batch
        self.nfe = 0
        self.k = [th.empty_like(y0) for _ in range(7)]      # f32, like torchdiffeq's k buffer: a bf16 model output is copied exactly
        if fused:
            np_ = 1 if parts is None else len(parts)
            self.ws = ops.ode_error_ratio_workspace(y0.numel(), y0.device)
            self.res = th.empty(np_, 2, dtype=th.float32, device=y0.device)
            self.host = th.empty(2 * np_, dtype=th.float32).pin_memory()

    def f(self, t32, y, slot):
        """k[slot] = drift(t, y); t goes to the model as th.full (== th.ones(B).to(x) * t without a blocking host copy)."""
        tv = th.full((self.batch,), float(t32), device=y.device, dtype=y.dtype)
        if self.fn_into_t is not None:
            self.fn_into_t(t32, tv, y, self.k[slot])
        elif self.fn_into is not None:
            self.fn_into(tv, y, self.k[slot])
        else:
            r = self.fn(tv, y)
            assert r.shape == y.shape, "Output shape from ODE solver must match input shape"
            self.k[slot].copy_(r)
        self.nfe += 1

    def norm(self, v):
        """torchdiffeq's norm: the RMS of a tensor state, _mixed_norm (max over the parts of their RMS) of a tuple state; a 0-d device tensor."""
        if self.parts is None:
            return _rms(v)
        return th.stack([_rms(v[a:b]) for a, b in self.parts]).max()

    def combine(self, y0, coef, dt, out):
        """out = y0 + sum_j (coef_j dt) k_j; y0 None: the sum alone."""
        cs = dopri5_weights(coef, dt)
        ks = self.k[:len(cs)]
        if self.fused:
            return ops.ode_rk_combine(y0, ks, cs, round_bf16=self.amp, out=out)
        s = None
        for c, k in zip(cs, ks):
            if self.amp:
                c, k = float(th.tensor(c).to(th.bfloat16)), k.to(th.bfloat16).float()
            s = c * k if s is None else s + c * k
        if self.amp:
            s = s.to(th.bfloat16).float()
        out.copy_(s if y0 is None else y0 + s)
        return out

    def error_ratio(self, y0, y1, dt):
        """-> (ratio, y1 holds a non-finite value) on the host: the one device -> host read of a step."""
        cs = dopri5_weights(DOPRI5_C_ERROR, dt)
        parts = [(0, y0.numel())] if self.parts is None else self.parts
        if self.fused:
            for p, (a, b) in enumerate(parts):
                sl = (lambda t: t) if self.parts is None else (lambda t, a=a, b=b: t[a:b])
                ops.ode_error_ratio(sl(y0), sl(y1), [sl(k) for k in self.k], cs, self.atol, self.rtol, round_bf16=self.amp, result=self.res[p], workspace=self.ws)
            self.host.copy_(self.res.view(-1), non_blocking=True)
            ev = th.cuda.Event()
            ev.record()
            ev.synchronize()
            flags = self.host.view(th.int32)
            return (max(float(np.sqrt(np.float64(self.host[2 * p].item()))) for p in range(len(parts))),
                    any(bool(flags[2 * p + 1].item()) for p in range(len(parts))))
        err = self.combine(None, DOPRI5_C_ERROR, dt, th.empty_like(y0))
        tol = self.atol + self.rtol * th.max(y0.abs(), y1.abs())
        e = err / tol
        ratios = []
        for a, b in parts:
            ep = e if self.parts is None else e[a:b]
            mean_sq = ep.double().pow(2).mean().float()         # the kernel's precision: f32 e, its squares summed in f64, the mean rounded to f32
            ratios.append(float(np.sqrt(np.float64(mean_sq.item()))))
        return max(ratios), not bool(th.isfinite(y1).all())

    def dense(self, y0, y1, ymid, dt, x, out):
        f0, f1 = self.k[0], self.k[6]
        if self.fused:
            return ops.ode_dense_output(y0, y1, ymid, f0, f1, dt, x, out=out)
        dt, x = float(np.float32(dt)), np.float32(x)          # Python floats holding f32 values: torch applies them in f32
        a = 2 * dt * (f1 - f0) - 8 * (y1 + y0) + 16 * ymid
        b = dt * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * ymid
        c = dt * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * ymid
        d = dt * f0
        total = y0 + float(x) * d
        xp = x
        for coef in (c, b, a):
            xp = np.float32(xp * x)
            total = total + float(xp) * coef
        out.copy_(total)
        return out

    def initial_dt(self, t0, y0):
        """_select_initial_step (order 5 - 1) with f0 = k[0] already evaluated; one more evaluation (k[1] holds it until the first stage)."""
        scale = self.atol + y0.abs() * self.rtol
        d0, d1 = (float(v) for v in th.stack([self.norm(y0 / scale), self.norm(self.k[0] / scale)]).tolist())
        h0 = dopri5_initial_h0(d0, d1)
        h32 = float(np.float32(h0))
        self.f(np.float32(t0 + h32), y0 + h32 * self.k[0], 1)
        d2 = float(self.norm((self.k[1] - self.k[0]) / scale)) / h0
        return dopri5_initial_dt(h0, d1, d2)

    def solve(self, y0, ts, max_num_steps):
        """-> [len(ts), *y0.shape]: out[0] = y0, then the dense output of the step covering each later grid time."""
        out = th.empty((len(ts), *y0.shape), dtype=y0.dtype, device=y0.device)
        out[0].copy_(y0)
        self.n_accepted = self.n_rejected = 0
        y, y1, ystage, ymid = y0.clone(), th.empty_like(y0), th.empty_like(y0), th.empty_like(y0)
        finite = bool(th.isfinite(y).all())
        t0 = ts[0]
        self.f(np.float32(t0), y, 0)
        dt = self.initial_dt(t0, y)
        i, steps = 1, 0
        while i < len(ts):
            if steps >= max_num_steps:
                raise RuntimeError(f"max_num_steps exceeded ({steps}>={max_num_steps})")
            if not finite:
                raise RuntimeError("non-finite values in state `y`")
            if not t0 + dt > t0:
                raise RuntimeError(f"underflow in dt {dt}")
            steps += 1
            times = dopri5_stage_times(t0, dt)
            for s, beta in enumerate(DOPRI5_BETA):
                yi = y1 if s == len(DOPRI5_BETA) - 1 else ystage       # the last stage's input is y1 (FSAL: its evaluation is the next f0)
                self.combine(y, beta, dt, yi)
                self.f(times[s], yi, s + 1)
            ratio, y1_bad = self.error_ratio(y, y1, dt)
            dt_next = dopri5_next_dt(dt, ratio)
            if dopri5_accept(ratio):
                self.n_accepted += 1
                t1 = t0 + dt
                todo = dopri5_pending_outputs(ts, i, t1)
                if len(todo):
                    self.combine(y, DOPRI5_C_MID, dt, ymid)
                    for j in todo:
                        self.dense(y, y1, ymid, np.float32(dt), dopri5_dense_x(ts[j], t0, t1), out[j])
                    i, steps = todo.stop, 0
                y, y1 = y1, y
                self.k[0], self.k[6] = self.k[6], self.k[0]
                t0, finite = t1, not y1_bad
            else:
                self.n_rejected += 1
            dt = dt_next
        return out


class ode:
    """integrators.py:79-118.  The reference hands the drift to `torchdiffeq.odeint`; that package is not a dependency, so the fixed-grid methods
    (torchdiffeq's fixed-grid set: explicit Euler, midpoint, Heun's third-order rule, the 3/8-rule RK4 -- one solver step per interval of the time grid; unpinned,
    there is no torchdiffeq here to compare against) and, for a CUDA f32 state, adaptive "dopri5" (the reference's default; `_Dopri5`) are
    integrated here, and anything else is delegated to torchdiffeq when it can be imported.  After a dopri5 call `nfe`, `n_accepted` and
    `n_rejected` hold its model evaluations and steps."""

    def __init__(self, drift, *, t0, t1, sampler_type, num_steps, atol, rtol, time_dist_shift=1.0, max_num_steps=2 ** 31 - 1, model_terms=None):
        assert t0 < t1, "ODE sampler has to be in forward time"
        self.drift = drift
        self.model_terms = model_terms      # te (CPU f32 [1, 1]) -> (kind, c0, dv, nsig) when `drift` is Transport.get_drift of a noise / score model, else None
        t = th.linspace(t0, t1, num_steps)
        self.t = 1 - time_dist_shift * (1 - t) / (1 + (time_dist_shift - 1) * (1 - t))
        self.atol, self.rtol = atol, rtol
        self.sampler_type = sampler_type
        self.max_num_steps = max_num_steps      # dopri5: attempted steps allowed per output interval (torchdiffeq's max_num_steps)
        self.nfe = self.n_accepted = self.n_rejected = 0      # dopri5's counters of the last call

    def _velocity_into(self, t32, tv, state, out, model, model_kwargs):
        """out = the drift of a noise / score model at (state, t): one forward and one kernel, its scalars from the host's f32 time t32.  The model's keywords
        come as a dict: the drivers pass the labels as `y`."""
        m = model(state, tv, **model_kwargs)
        assert m.shape == state.shape, "Output shape from ODE solver must match input shape"
        return ops.model_velocity(state, m.contiguous(), self.model_terms(th.tensor(float(t32), dtype=th.float32).view(1, 1)), out=out)

    def _dopri5(self, x, model, **model_kwargs):
        """dopri5 on a CUDA f32 state; the output is stacked [num_steps, ...] like odeint's."""
        into = None
        if FUSED_STATE_UPDATE and self.model_terms is not None:      # k[slot] straight from the conversion kernel
            into = lambda t32, tv, y, out: self._velocity_into(t32, tv, y, out, model, model_kwargs)
        solver = _Dopri5(lambda t, y: self.drift(y, t, model, **model_kwargs), x, atol=self.atol, rtol=self.rtol, fused=FUSED_STATE_UPDATE,
                         round_bf16=th.is_autocast_enabled(), fn_into_t=into)
        try:
            with th.no_grad():
                return solver.solve(x.contiguous(), self.t.double().tolist(), self.max_num_steps)
        finally:
            self.nfe, self.n_accepted, self.n_rejected = solver.nfe, getattr(solver, "n_accepted", 0), getattr(solver, "n_rejected", 0)

    def _flat(self, x, model, **model_kwargs):
        """A tuple state as one flat f32 buffer (torchdiffeq's _TupleFunc: the flattened parts concatenated) -> (buffer, its [start, stop) parts, unflatten
        of a stacked [T, n] result into the tuple, fn_into(t, y, out) writing the drift of the flat state y into the flat slot out).  A drift with a `packed`
        form (Sampler.sample_ode_likelihood's: one kernel for the whole slot) uses it when FUSED_STATE_UPDATE is set."""
        shapes = [p.shape for p in x]
        bounds, a = [], 0
        for p in x:
            bounds.append((a, a + p.numel()))
            a += p.numel()
        y0 = th.cat([p.reshape(-1) for p in x])
        views = lambda y: tuple(y[a:b].view(sh) for (a, b), sh in zip(bounds, shapes))
        packed = getattr(self.drift, "packed", None)
        if FUSED_STATE_UPDATE and packed is not None:
            def fn_into(t, y, out):
                packed(views(y), t, model, out=out, **model_kwargs)
        else:
            def fn_into(t, y, out):
                r = self.drift(views(y), t, model, **model_kwargs)
                for (a, b), sh, r_ in zip(bounds, shapes, r):
                    assert r_.shape == sh, "Output shape from ODE solver must match input shape"
                    out[a:b].copy_(r_.reshape(-1))
        unflat = lambda ys: tuple(ys[:, a:b].reshape(ys.shape[0], *sh) for (a, b), sh in zip(bounds, shapes))
        return y0, bounds, unflat, fn_into

    def _dopri5_tuple(self, x, model, **model_kwargs):
        """dopri5 on a tuple of CUDA f32 tensors (the likelihood sampler's (x, logp)) held as one flat buffer; the output is the tuple of the parts'
        [num_steps, ...] trajectories."""
        y0, bounds, unflat, fn_into = self._flat(x, model, **model_kwargs)
        solver = _Dopri5(None, y0, atol=self.atol, rtol=self.rtol, fused=FUSED_STATE_UPDATE, round_bf16=th.is_autocast_enabled(), parts=bounds,
                         batch=x[0].size(0), fn_into=fn_into)
        try:
            with th.no_grad():
                return unflat(solver.solve(y0, self.t.double().tolist(), self.max_num_steps))
        finally:
            self.nfe, self.n_accepted, self.n_rejected = solver.nfe, getattr(solver, "n_accepted", 0), getattr(solver, "n_rejected", 0)

    def sample(self, x, model, **model_kwargs):
        if self.sampler_type == "dopri5" and not isinstance(x, tuple) and x.is_cuda and x.dtype == th.float32:
            return self._dopri5(x, model, **model_kwargs)
        on_device = isinstance(x, tuple) and all(p.is_cuda and p.dtype == th.float32 for p in x)
        if on_device and self.sampler_type == "dopri5":
            return self._dopri5_tuple(x, model, **model_kwargs)
        device = x[0].device if isinstance(x, tuple) else x.device

        def fn(t, x, tc=None):      # tc: the CPU twin of the device time t (the kernel route's scalars come from it)
            n = x[0].size(0) if isinstance(x, tuple) else x.size(0)
            return self.drift(x, _time_vector(n, t, device=device), model, **model_kwargs)

        t = self.t.to(device)
        if self.sampler_type not in _FIXED_GRID:
            try:
                from torchdiffeq import odeint
            except ImportError as e:
                raise NotImplementedError(f"ODE method {self.sampler_type!r} needs torchdiffeq (not installed); fixed-grid methods available: "
                                          f"{_FIXED_GRID}") from e
            k = len(x) if isinstance(x, tuple) else 1
            return odeint(fn, x, t, method=self.sampler_type, atol=[self.atol] * k, rtol=[self.rtol] * k)
        unflat = None
        if isinstance(x, tuple):
            if not on_device:
                raise NotImplementedError("tuple states (the likelihood sampler) are built for CUDA f32 tensors only")
            batch = x[0].size(0)
            x, _, unflat, fn_into = self._flat(x, model, **model_kwargs)      # elementwise methods: they run on the flat buffer as they stand

            def fn(t, y, tc=None):
                out = th.empty_like(y)
                fn_into(_time_vector(batch, t, device=device), y, out)
                return out
        elif FUSED_STATE_UPDATE and self.model_terms is not None and x.is_cuda and x.dtype == th.float32:
            def fn(t, x, tc):       # a noise / score model: one forward and the conversion kernel; the model's time vector is filled from the host's number too
                return self._velocity_into(tc, _time_vector(x.size(0), float(tc), device=device), x.contiguous(), None, model, model_kwargs)
        out = [x]
        tc = self.t                 # the grid on the CPU: the kernel route takes its scalars AND the model's time vector from this twin (no device read; the device's
                                    # own stage times, where a division by a Python number may be a multiplication by its reciprocal, are not used on that route)
        with th.no_grad():
            for i in range(t.numel() - 1):
                t0, dt = t[i], t[i + 1] - t[i]
                c0, cdt = tc[i], tc[i + 1] - tc[i]
                k1 = fn(t0, x, c0)
                if self.sampler_type == "euler":
                    x = x + dt * k1
                elif self.sampler_type == "midpoint":
                    x = x + dt * fn(t0 + 0.5 * dt, x + 0.5 * dt * k1, c0 + 0.5 * cdt)
                elif self.sampler_type == "heun3":
                    k2 = fn(t0 + dt / 3, x + dt * k1 / 3, c0 + cdt / 3)
                    k3 = fn(t0 + dt * 2 / 3, x + dt * k2 * (2 / 3), c0 + cdt * 2 / 3)
                    x = x + dt * (0.25 * k1 + 0.75 * k3)
                else:                                                    # rk4, 3/8 rule
                    k2 = fn(t0 + dt / 3, x + dt * k1 / 3, c0 + cdt / 3)
                    k3 = fn(t0 + dt * 2 / 3, x + dt * (k2 - k1 / 3), c0 + cdt * 2 / 3)
                    k4 = fn(t0 + dt, x + dt * (k1 - k2 + k3), c0 + cdt)
                    x = x + dt * (k1 + 3 * (k2 + k3) + k4) * 0.125
                out.append(x)
        return th.stack(out) if unflat is None else unflat(th.stack(out))


class Sampler:
    """transport.py:223-459 (`sample_sde`, `sample_ode`, `sample_ode_likelihood`)."""

    def __init__(self, transport: Transport):
        self.transport = transport
        self.drift = transport.get_drift()
        self.score = transport.get_score()

    def _sde_diffusion_and_drift(self, *, diffusion_form="SBDM", diffusion_norm=1.0):
        ps = self.transport.path_sampler

        def diffusion_fn(x, t):
            return ps.compute_diffusion(x, t, form=diffusion_form, norm=diffusion_norm)

        def sde_drift(x, t, model, **kw):
            temp = self.drift(x, t, model, **kw)
            return temp + diffusion_fn(x, t) * self.transport.convert_score(temp, x, t)

        return sde_drift, diffusion_fn

    def _last_step(self, sde_drift, *, last_step, last_step_size, t1, fused=None):
        """transport.py:275-295.  `t1`: the last step's time as the host knows it; the kernel routes form their coefficients from it, not from the `t` they are
        called with -- reading that back waits for the model evaluation queued before it and leaves the device idle until the kernel is launched."""
        ps = self.transport.path_sampler
        te = th.tensor([t1], dtype=th.float32).view(1, 1)      # the value `th.ones(n, device=...) * t1` holds
        if last_step is None:
            return lambda x, t, model, **kw: x
        on_kernel = lambda x: FUSED_STATE_UPDATE and fused is not None and x.is_cuda and x.dtype == th.float32
        mt = fused[3] if fused is not None and len(fused) > 3 else ModelType.VELOCITY
        # What the kernels consume: a velocity model's drift (terms None), or a noise / score model's output itself with the prologue scalars, formed on the kernel route only
        if mt == ModelType.VELOCITY:
            terms, output = (lambda: None), self.drift
        else:
            terms, output = (lambda: model_terms(ps, mt, te)), (lambda x, t, model, **kw: model(x, t, **kw))
        if last_step == "Mean":
            def mean_step(x, t, model, **kw):
                if on_kernel(x):
                    rar, var = ps._score_coeffs(te)
                    diff = float(ps.compute_diffusion(te, te.view(1), form=fused[1], norm=fused[2]))
                    return ops.sde_euler_step(x.contiguous(), output(x, t, model, **kw).contiguous(), None, float(rar), float(var), diff, float(last_step_size),
                                              0.0, 0.0, terms=terms())[0]
                return x + sde_drift(x, t, model, **kw) * last_step_size
            return mean_step
        if last_step == "Tweedie":
            alpha, sigma = ps.compute_alpha_t, ps.compute_sigma_t

            def tweedie_step(x, t, model, **kw):
                if on_kernel(x):          # with terms, Transport.get_score: the model's own score, not the one converted from the velocity (rar, var unused)
                    rar, var = ps._score_coeffs(te)
                    a = alpha(te)[0]
                    return ops.sde_last_step(x.contiguous(), output(x, t, model, **kw).contiguous(), ops.LAST_STEP_TWEEDIE, a=float(a),
                                             c=float((sigma(te)[0] ** 2) / a), rar=float(rar), var=float(var), terms=terms())
                return x / alpha(t)[0][0] + (sigma(t)[0][0] ** 2) / alpha(t)[0][0] * self.score(x, t, model, **kw)
            return tweedie_step
        if last_step == "Euler":
            def euler_step(x, t, model, **kw):
                if on_kernel(x):
                    return ops.sde_last_step(x.contiguous(), output(x, t, model, **kw).contiguous(), ops.LAST_STEP_EULER, h=float(last_step_size), terms=terms())
                return x + self.drift(x, t, model, **kw) * last_step_size
            return euler_step
        raise NotImplementedError()

    def sample_sde(self, *, sampling_method="Euler", diffusion_form="SBDM", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04, num_steps=250):
        """-> `sample_fn(init, model, **model_kwargs)` returning the list of `num_steps` states (transport.py:298-354)."""
        if last_step is None:
            last_step_size = 0.0
        sde_drift, sde_diffusion = self._sde_diffusion_and_drift(diffusion_form=diffusion_form, diffusion_norm=diffusion_norm)
        t0, t1 = self.transport.check_interval(self.transport.train_eps, self.transport.sample_eps, diffusion_form=diffusion_form, sde=True, eval=True,
                                               reverse=False, last_step_size=last_step_size)
        fused = (self.transport.path_sampler, diffusion_form, diffusion_norm, self.transport.model_type)
        _sde = sde(sde_drift, sde_diffusion, t0=t0, t1=t1, num_steps=num_steps, sampler_type=sampling_method, fused=fused)
        last_step_fn = self._last_step(sde_drift, last_step=last_step, last_step_size=last_step_size, t1=t1, fused=fused)

        def _sample(init, model, **model_kwargs):
            xs = _sde.sample(init, model, **model_kwargs)
            ts = th.ones(init.size(0), device=init.device) * t1
            xs.append(last_step_fn(xs[-1], ts, model, **model_kwargs))
            assert len(xs) == num_steps, "Samples does not match the number of steps"
            return xs

        return _sample

    def sample_ode(self, *, sampling_method="dopri5", num_steps=50, atol=1e-6, rtol=1e-3, reverse=False):
        """transport.py:356-407."""
        if reverse:
            drift = lambda x, t, model, **kw: self.drift(x, th.ones_like(t) * (1 - t), model, **kw)
        else:
            drift = self.drift
        t0, t1 = self.transport.check_interval(self.transport.train_eps, self.transport.sample_eps, sde=False, eval=True, reverse=reverse,
                                               last_step_size=0.0)
        terms = None          # a noise / score model in forward time: the drift's conversion is one kernel per evaluation (ode._velocity_into)
        if self.transport.model_type != ModelType.VELOCITY and not reverse:
            terms = lambda te: model_terms(self.transport.path_sampler, self.transport.model_type, te)
        return ode(drift=drift, t0=t0, t1=t1, sampler_type=sampling_method, num_steps=num_steps, atol=atol, rtol=rtol,
                   time_dist_shift=self.transport.time_dist_shift, model_terms=terms).sample

    def sample_ode_likelihood(self, *, sampling_method="dopri5", num_steps=50, atol=1e-6, rtol=1e-3):
        """transport.py:402-459 -> `_sample_fn(x, model, **model_kwargs)` returning (logp [B], z): the probability-flow ODE from the data (model time 1) to the
        prior (model time 0) on the state (x, delta_logp), with the divergence of the drift estimated by Hutchinson's trick -- d logp / dt = eps^T J eps, one
        Rademacher probe eps per evaluation, the VJP g = J^T eps from autograd -- and logp = prior_logp(z) - delta_logp at the last grid time.
        The reference evaluates the model twice per drift call (once inside autograd.grad, once more for the drift itself); here the drift is the output of
        the forward whose graph gives the VJP (the same values: the second call repeats the first).  On a CUDA f32 state the (x, logp) tuple is one flat
        buffer (`ode._dopri5_tuple`) and each evaluation's stage value comes from one kernel (`ops.ode_hutchinson_pack`).  After a call `_sample_fn.ode` holds
        the solver's `nfe`, `n_accepted` and `n_rejected`.  For a noise / score model the drift stays the tensor-op composition of `Transport.get_drift`:
        autograd needs the VJP through the conversion."""
        drift_fn = self.drift

        def _vjp(x, t, model, **kw):
            """-> (v, g, eps): the drift at (x, 1 - t), the gradient of sum(v * eps) with respect to x, the probe -- eps drawn by the reference's own call,
            so a seeded run consumes the device generator as the reference does."""
            eps = th.randint(2, x.size(), dtype=th.float, device=x.device) * 2 - 1
            t = th.ones_like(t) * (1 - t)
            with th.enable_grad():
                x = x.detach().requires_grad_(True)
                v = drift_fn(x, t, model, **kw)
                grad = th.autograd.grad(th.sum(v * eps), x)[0]
            return v.detach(), grad, eps

        def _likelihood_drift(x, t, model, **kw):
            x, _ = x
            v, grad, eps = _vjp(x, t, model, **kw)
            return (-v, th.sum(grad * eps, dim=tuple(range(1, len(x.size())))))

        def _packed(x, t, model, out, **kw):
            """The same stage value written into the flat slot `out` ([n_x + B] f32) by one kernel: out[:n_x] = -v, out[n_x + b] = sum_i g * eps."""
            x, _ = x
            v, grad, eps = _vjp(x, t, model, **kw)
            ops.ode_hutchinson_pack(v.contiguous(), grad.float().contiguous(), eps, out=out)

        _likelihood_drift.packed = _packed
        t0, t1 = self.transport.check_interval(self.transport.train_eps, self.transport.sample_eps, sde=False, eval=True, reverse=False,
                                               last_step_size=0.0)
        _ode = ode(drift=_likelihood_drift, t0=t0, t1=t1, sampler_type=sampling_method, num_steps=num_steps, atol=atol, rtol=rtol)

        def _sample_fn(x, model, **model_kwargs):
            init_logp = th.zeros(x.size(0)).to(x)
            drift, delta_logp = _ode.sample((x, init_logp), model, **model_kwargs)
            drift, delta_logp = drift[-1], delta_logp[-1]
            prior_logp = self.transport.prior_logp(drift)
            logp = prior_logp - delta_logp
            return logp, drift

        _sample_fn.ode = _ode
        return _sample_fn
