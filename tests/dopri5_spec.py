"""The dopri5 ODE method the reference's `Sampler.sample_ode` defaults to (diffusion/transport/transport.py:356-407 -> torchdiffeq.odeint,
diffusion/transport/integrators.py:79-118), restated in float64: torchdiffeq 0.2.x's RKAdaptiveStepsizeODESolver with the Dormand-Prince-Shampine
tableau -- initial step, Runge-Kutta step with FSAL, error ratio, step-size controller, quartic dense output.  The tableau is held as exact
fractions.  A plain helper module for tests/test_oracle_dopri5.py and tests/test_gpu_ode_dopri5.py (unpinned: torchdiffeq is not a dependency)."""
from fractions import Fraction as F

import numpy as np

ALPHA = [F(1, 5), F(3, 10), F(4, 5), F(8, 9), F(1), F(1)]
BETA = [[F(1, 5)],
        [F(3, 40), F(9, 40)],
        [F(44, 45), F(-56, 15), F(32, 9)],
        [F(19372, 6561), F(-25360, 2187), F(64448, 6561), F(-212, 729)],
        [F(9017, 3168), F(-355, 33), F(46732, 5247), F(49, 176), F(-5103, 18656)],
        [F(35, 384), F(0), F(500, 1113), F(125, 192), F(-2187, 6784), F(11, 84)]]
B_SOL = BETA[-1] + [F(0)]                       # FSAL: y1 is the 7th stage's input
B_HAT = [F(1951, 21600), F(0), F(22642, 50085), F(451, 720), F(-12231, 42400), F(649, 6300), F(1, 60)]
C_ERR = [b - bh for b, bh in zip(B_SOL, B_HAT)]
C_MID = [F(6025192743, 30085553152) / 2, F(0), F(51252292925, 65400821598) / 2, F(-2691868925, 45128329728) / 2,
         F(187940372067, 1594534317056) / 2, F(-1776094331, 19743644256) / 2, F(11237099, 235043384) / 2]
C_NODES = [F(0)] + ALPHA                        # the node of stage j (k_j)


def rms(v):
    return float(np.sqrt(np.mean(np.square(v))))


def initial_h0(d0, d1):
    return 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1


def initial_dt_from(h0, d1, d2):
    h1 = max(1e-6, h0 * 1e-3) if d1 <= 1e-15 and d2 <= 1e-15 else (0.01 / max(d1, d2)) ** (1 / 5)
    return min(100 * h0, h1)


def next_dt(dt, ratio):
    if ratio == 0:
        return dt * 10
    dfactor = 1.0 if ratio < 1 else 0.2
    return dt * min(10.0, max(0.9 * ratio ** (-1 / 5), dfactor))


def weighted(k, coef):
    return sum(float(c) * kj for c, kj in zip(coef, k))


def solve(f, y0, ts, atol, rtol, max_attempts=100000):
    """f(t, y) -> dy/dt (float64 arrays).  -> (out [len(ts), *y0.shape], steps [(t0, dt, ratio, accepted)], nfe)."""
    nfe = [0]

    def fe(t, y):
        nfe[0] += 1
        return f(t, y)

    y0 = np.asarray(y0, dtype=np.float64)
    out = [y0]
    t0, y, f0 = float(ts[0]), y0, fe(float(ts[0]), y0)
    scale = atol + rtol * np.abs(y)
    d0, d1 = rms(y / scale), rms(f0 / scale)
    h0 = initial_h0(d0, d1)
    f1 = fe(t0 + h0, y + h0 * f0)
    dt = initial_dt_from(h0, d1, rms((f1 - f0) / scale) / h0)
    steps, i = [], 1
    while i < len(ts):
        assert len(steps) < max_attempts and t0 + dt > t0 and np.isfinite(y).all()
        k = [f0]
        for a, beta in zip(ALPHA, BETA):
            yi = y + dt * weighted(k, beta)
            k.append(fe(t0 + float(a) * dt, yi))
        y1 = yi
        err = dt * weighted(k, C_ERR)
        ratio = rms(err / (atol + rtol * np.maximum(np.abs(y), np.abs(y1))))
        accept = ratio <= 1
        steps.append((t0, dt, ratio, accept))
        if accept:
            t1 = t0 + dt
            ymid = y + dt * weighted(k, C_MID)
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
        dt = next_dt(dt, ratio)
    return np.stack(out), steps, nfe[0]
