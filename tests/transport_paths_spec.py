"""The sampler's graph for any model type on the Linear, GVP and VP paths, written out op by op on CPU tensors with the reference's broadcasting (t as a
[B, 1, ...] f32 tensor next to the model's output m, which may be bf16), so PyTorch's own type promotion decides every rounding site:

  coefficients  alpha, d_alpha, sigma, d_sigma, d_alpha / alpha and the drift of each path (path.py:23-43, 149-171, 178-192), each expression as the
                reference writes it, evaluated on the CPU,
  velocity      m for a velocity model, else (-drift_mean) + drift_var * score (transport.py:171-181) with score = m / -sigma (noise) or m (score): f32
                whatever m is,
  own_score     Transport.get_score (transport.py:202-216): m / -sigma (f32), m itself (m's type), or the score converted from a velocity,

and the sampler steps built on them (integrators.py:27-48, transport.py:253-256, 275-288).  tests/test_gpu_transport_paths.py holds each kernel of
csrc/sampler.hip to these functions bit for bit; tests/test_transport_paths_cpu.py holds the host's scalar form (`transport.model_terms`) to them."""
import numpy as np
import torch

from oracle import ref_cpu as R

NOISE, SCORE, VELOCITY = "noise", "score", "velocity"
LINEAR, GVP, VP = "Linear", "GVP", "VP"
VP_MIN, VP_MAX = 0.1, 20.0


def _log_mean(t):
    return -0.25 * ((1 - t) ** 2) * (VP_MAX - VP_MIN) - 0.5 * (1 - t) * VP_MIN


def _d_log_mean(t):
    return 0.5 * (1 - t) * (VP_MAX - VP_MIN) + 0.5 * VP_MIN


def alpha(te, path=LINEAR):
    """-> (alpha_t, d_alpha_t)."""
    if path == LINEAR:
        return te, 1
    if path == GVP:
        return torch.sin(te * np.pi / 2), np.pi / 2 * torch.cos(te * np.pi / 2)
    a = torch.exp(_log_mean(te))
    return a, a * _d_log_mean(te)


def sigma(te, path=LINEAR):
    """-> (sigma_t, d_sigma_t)."""
    if path == LINEAR:
        return 1 - te, -1
    if path == GVP:
        return torch.cos(te * np.pi / 2), -np.pi / 2 * torch.sin(te * np.pi / 2)
    p = 2 * _log_mean(te)
    s = torch.sqrt(1 - torch.exp(p))
    return s, torch.exp(p) * (2 * _d_log_mean(te)) / (-2 * s)


def ratio(te, path=LINEAR):
    if path == LINEAR:
        return 1 / te
    if path == GVP:
        return np.pi / (2 * torch.tan(te * np.pi / 2))
    return _d_log_mean(te)


def drift(x, te, path=LINEAR):
    """-> (drift_mean, drift_var) of compute_drift."""
    if path == VP:
        beta = VP_MIN + (1 - te) * (VP_MAX - VP_MIN)
        return -0.5 * beta * x, beta / 2
    r = ratio(te, path)
    s, ds = sigma(te, path)
    return -(r * x), r * (s ** 2) - s * ds


def diffusion(x, te, form, norm, path=LINEAR):
    if form == "constant":
        return norm
    if form == "SBDM":
        return norm * drift(x, te, path)[1]
    if form == "sigma":
        return norm * sigma(te, path)[0]
    if form == "linear":
        return norm * (1 - te)
    raise NotImplementedError(form)


def score_from_velocity(v, x, te, path=LINEAR):
    a, da = alpha(te, path)
    s, ds = sigma(te, path)
    rar = a / da
    var = s ** 2 - rar * ds * s
    return (rar * v - x) / var


def own_score(kind, m, x, t, path=LINEAR):
    te = R.expand_t(t, x)
    if kind == NOISE:
        return m / -sigma(te, path)[0]
    if kind == SCORE:
        return m
    return score_from_velocity(m, x, te, path)


def velocity(kind, m, x, t, path=LINEAR):
    if kind == VELOCITY:
        return m
    te = R.expand_t(t, x)
    drift_mean, drift_var = drift(x, te, path)
    s = m / -sigma(te, path)[0] if kind == NOISE else m
    return -drift_mean + drift_var * s


def sde_drift(kind, m, x, t, form, norm, path=LINEAR):
    te = R.expand_t(t, x)
    v = velocity(kind, m, x, t, path)
    return v + diffusion(x, te, form, norm, path) * score_from_velocity(v, x, te, path)


def euler_step(kind, x, m, w, t, dt, form, norm, path=LINEAR):
    """-> (x_new, mean_x); w None: the "Mean" last step with dt = last_step_size (a Python float there)."""
    mean = x + sde_drift(kind, m, x, t, form, norm, path) * dt
    if w is None:
        return mean, mean
    return mean + torch.sqrt(2 * diffusion(x, R.expand_t(t, x), form, norm, path)) * (w * torch.sqrt(dt)), mean


def heun_perturb(x, w, t, dt, form, norm, path=LINEAR):
    return x + torch.sqrt(2 * diffusion(x, R.expand_t(t, x), form, norm, path)) * (w * torch.sqrt(dt))


def heun_predict(kind, xhat, m1, t, dt, form, norm, path=LINEAR):
    k1 = sde_drift(kind, m1, xhat, t, form, norm, path)
    return k1, xhat + dt * k1


def heun_correct(kind, xhat, xp, k1, m2, t2, dt, form, norm, path=LINEAR):
    return xhat + 0.5 * dt * (k1 + sde_drift(kind, m2, xp, t2, form, norm, path))


def tweedie(kind, x, m, t, path=LINEAR):
    """transport.py:279-284: alpha(t)[0][0] and sigma(t)[0][0] are 0-d tensors, so for a bf16 score model the product with m stays bf16."""
    a, s = alpha(t, path)[0][0], sigma(t, path)[0][0]
    return x / a + (s ** 2) / a * own_score(kind, m, x, t, path)


def euler_last(kind, x, m, t, h, path=LINEAR):
    return x + velocity(kind, m, x, t, path) * h
