"""tests/dopri5_spec.py extended to tuple states, in float64: torchdiffeq 0.2.x holds a tuple state as ONE flat buffer (_TupleFunc: the flattened parts
concatenated) and measures it with its default tuple norm, _mixed_norm -- the max over the parts of each part's RMS -- in _select_initial_step (d0, d1, d2)
and in _compute_error_ratio.  What the reference's `Sampler.sample_ode_likelihood` (diffusion/transport/transport.py:402-459) integrates: (x, logp).
A plain helper module for tests/test_oracle_ode_likelihood.py and tests/test_gpu_ode_likelihood.py (unpinned: torchdiffeq is not a dependency)."""
import numpy as np

import dopri5_spec as S


def mixed_norm(parts):
    """The norm of a flat state cut at `parts` ([start, stop) ranges): max over the parts of their RMS."""
    return lambda v: max(S.rms(v[a:b]) for a, b in parts)


def solve(f, y0, ts, atol, rtol, parts=None, max_attempts=100000):
    """dopri5_spec.solve with the norm of a tuple state: f(t, y) -> dy/dt on the flat float64 buffer y; parts None: the flat RMS (a single tensor).
    -> (out [len(ts), n], steps [(t0, dt, ratio, accepted)], nfe)."""
    norm = S.rms if parts is None else mixed_norm(parts)
    nfe = [0]

    def fe(t, y):
        nfe[0] += 1
        return f(t, y)

    y0 = np.asarray(y0, dtype=np.float64)
    out = [y0]
    t0, y, f0 = float(ts[0]), y0, fe(float(ts[0]), y0)
    scale = atol + rtol * np.abs(y)
    d0, d1 = norm(y / scale), norm(f0 / scale)
    h0 = S.initial_h0(d0, d1)
    f1 = fe(t0 + h0, y + h0 * f0)
    dt = S.initial_dt_from(h0, d1, norm((f1 - f0) / scale) / h0)
    steps, i = [], 1
    while i < len(ts):
        assert len(steps) < max_attempts and t0 + dt > t0 and np.isfinite(y).all()
        k = [f0]
        for a, beta in zip(S.ALPHA, S.BETA):
            yi = y + dt * S.weighted(k, beta)
            k.append(fe(t0 + float(a) * dt, yi))
        y1 = yi
        err = dt * S.weighted(k, S.C_ERR)
        ratio = norm(err / (atol + rtol * np.maximum(np.abs(y), np.abs(y1))))
        accept = ratio <= 1
        steps.append((t0, dt, ratio, accept))
        if accept:
            t1 = t0 + dt
            ymid = y + dt * S.weighted(k, S.C_MID)
            fa, fb = k[0], k[-1]
            a = 2 * dt * (fb - fa) - 8 * (y1 + y) + 16 * ymid
            b = dt * (5 * fa - 3 * fb) + 18 * y + 14 * y1 - 32 * ymid
            c = dt * (fb - 4 * fa) - 11 * y - 5 * y1 + 16 * ymid
            d = dt * fa
            while i < len(ts) and ts[i] <= t1:
                x = (ts[i] - t0) / (t1 - t0)
                out.append(y + x * d + x ** 2 * c + x ** 3 * b + x ** 4 * a)
                i += 1
            t0, y, f0 = t1, y1, k[-1]
        dt = S.next_dt(dt, ratio)
    return np.stack(out), steps, nfe[0]


# ---- Gaussian data: the exact linear-path velocity and likelihood ----------------------------------------------------------------------------------------
# data x1 ~ N(0, s^2 I), noise x0 ~ N(0, I), x_t = t x1 + (1 - t) x0 (the Linear path, velocity prediction): E[x1 - x0 | x_t = x] = x * a(t) with
# a(t) = (t s^2 - (1 - t)) / (t^2 s^2 + (1 - t)^2).  Its Jacobian a(t) I is diagonal, so Rademacher Hutchinson is exact: eps^T J eps = D a(t) for every eps.


def gaussian_rate(t, s):
    return (t * s * s - (1 - t)) / (t * t * s * s + (1 - t) ** 2)


def gaussian_likelihood_drift(s, d, batch):
    """The likelihood sampler's drift on the flat state [x (batch * d) | logp (batch)] at solver time u (model time 1 - u): (-v, eps^T J eps)."""
    nx = batch * d

    def f(u, y):
        a = gaussian_rate(1 - u, s)
        return np.concatenate([-a * y[:nx], np.full(batch, d * a)])
    return f


def gaussian_logp(x, s):
    """Closed form: log N(x; 0, s^2 I) per sample of x [B, D], and z = x / s."""
    d = x.shape[1]
    return -d / 2 * np.log(2 * np.pi * s * s) - (x ** 2).sum(1) / (2 * s * s), x / s
