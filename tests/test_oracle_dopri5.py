"""The dopri5 ODE sampler (the reference's default `sample_ode` method: transport.py:356-407 -> torchdiffeq.odeint, integrators.py:79-118) on the CPU:
the float64 restatement of tests/dopri5_spec.py checked against scipy's RK45 tableau, the order conditions and analytic solutions, and the host logic of
`dmvae_amd.transport` (controller, initial step, grid bookkeeping and the composed tensor-op route) against the restatement."""
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import dopri5_spec as S

ATOL, RTOL = 1e-6, 1e-3
# y' = lam(t) y with lam(t) = -1 + 6 cos(20 t): 16 attempted steps on the shifted 50-point grid, 6 of them rejected, no error ratio within 0.35 of 1
LAM = (1.0, 6.0, 20.0)


def shifted_grid(num_steps=50, shift=2.5):
    from dmvae_amd.transport import ode
    return ode(None, t0=0, t1=1, sampler_type="dopri5", num_steps=num_steps, atol=ATOL, rtol=RTOL, time_dist_shift=shift).t.double().tolist()


def lam_problem(a=LAM[0], b=LAM[1], om=LAM[2]):
    lam = lambda t: -a + b * np.cos(om * t)
    big = lambda t: -a * t + b / om * np.sin(om * t)
    return lam, lambda y0, t, t0: y0 * np.exp(big(t) - big(t0))


def test_tableau_matches_scipy_rk45():
    from scipy.integrate._ivp.rk import RK45
    assert np.array_equal(RK45.C, [0.0] + [float(a) for a in S.ALPHA[:5]])
    for i in range(1, 6):
        assert np.array_equal(RK45.A[i, :i], [float(b) for b in S.BETA[i - 1]]), i
        assert not RK45.A[i, i:].any()
    assert np.array_equal(RK45.B, [float(b) for b in S.BETA[-1]])
    assert S.B_SOL[:6] == S.BETA[-1] and S.B_SOL[6] == 0 and S.ALPHA[4] == S.ALPHA[5] == 1
    # the error weights are b - b_hat with Shampine's b_hat, NOT scipy's classic embedded pair
    assert not np.allclose(RK45.E, [-float(c) for c in S.C_ERR], rtol=1e-3, atol=0)


def test_embedded_weights_order_conditions():
    c, A = S.C_NODES, [[]] + S.BETA

    def Av(v):
        return [sum((A[i][j] * v[j] for j in range(len(A[i]))), F(0)) for i in range(7)]

    dot = lambda w, v: sum((wi * vi for wi, vi in zip(w, v)), F(0))
    ones = [F(1)] * 7
    c2, c3 = [x ** 2 for x in c], [x ** 3 for x in c]
    Ac = Av(c)
    for w in (S.B_HAT, S.B_SOL):
        assert dot(w, ones) == 1 and dot(w, c) == F(1, 2)
        assert dot(w, c2) == F(1, 3) and dot(w, Ac) == F(1, 6)
        assert dot(w, c3) == F(1, 4) and dot(w, [x * y for x, y in zip(c, Ac)]) == F(1, 8)
        assert dot(w, Av(c2)) == F(1, 12) and dot(w, Av(Ac)) == F(1, 24)
    assert sum(S.C_ERR) == 0
    # the row sums of A are the nodes
    assert all(sum(A[i], F(0)) == c[i] for i in range(1, 7))


def test_mid_point_weights():
    for k in range(4):
        assert sum(m * x ** k for m, x in zip(S.C_MID, S.C_NODES)) == F(1, 2) ** (k + 1) / (k + 1), k


@pytest.mark.parametrize("case", ["decay", "growth", "lam_t", "rotation"])
def test_spec_against_exact_solutions(case):
    ts = shifted_grid()
    y0 = np.linspace(-1, 1, 14).reshape(2, 7) + 0.05
    if case == "rotation":
        w = 5.0
        y0 = np.array([[1.0, 0.0], [0.3, -0.7], [-0.4, 0.2]])
        f = lambda t, y: np.stack([-w * y[..., 1], w * y[..., 0]], -1)

        def exact(t):
            th_ = w * (t - ts[0])
            return np.stack([y0[:, 0] * np.cos(th_) - y0[:, 1] * np.sin(th_), y0[:, 0] * np.sin(th_) + y0[:, 1] * np.cos(th_)], -1)
    elif case == "lam_t":
        lam, sol = lam_problem()
        f = lambda t, y: lam(t) * y
        exact = lambda t: sol(y0, t, ts[0])
    else:
        r = -1.0 if case == "decay" else 1.5
        f = lambda t, y: r * y
        exact = lambda t: y0 * np.exp(r * (t - ts[0]))
    out, steps, nfe = S.solve(f, y0, ts, ATOL, RTOL)
    assert out.shape == (50,) + y0.shape and np.array_equal(out[0], y0)
    ex = np.stack([exact(t) for t in ts])
    bound = ATOL + RTOL * np.abs(ex).max()
    assert np.abs(out - ex).max() < 10 * bound, np.abs(out - ex).max() / bound
    assert nfe == 2 + 6 * len(steps)
    if case == "lam_t":
        assert sum(not s[3] for s in steps) >= 3            # the controller's reject branch is exercised


def test_host_controller_functions_equal_the_spec():
    from dmvae_amd import transport as T
    for d0, d1 in [(0.0, 1.0), (3.0, 2e-6), (1e3, 7.0), (12.5, 0.3)]:
        assert T.dopri5_initial_h0(d0, d1) == S.initial_h0(d0, d1)
    for h0, d1, d2 in [(1e-6, 0.0, 0.0), (1e-3, 5.0, 700.0), (0.02, 1e-16, 1e-17), (4e-4, 30.0, 2.0)]:
        assert T.dopri5_initial_dt(h0, d1, d2) == pytest.approx(S.initial_dt_from(h0, d1, d2), rel=1e-15)
    for dt, ratio in [(0.1, 0.0), (0.1, 1e-8), (0.05, 0.7), (0.05, 1.0), (0.02, 1.3), (0.3, 40.0), (1e-3, 1e9)]:
        assert T.dopri5_next_dt(dt, ratio) == pytest.approx(S.next_dt(dt, ratio), rel=1e-15)
        assert T.dopri5_accept(ratio) == (ratio <= 1)
    assert T.dopri5_next_dt(0.1, float("nan")) != T.dopri5_next_dt(0.1, float("nan"))
    for j, (a, b) in enumerate(zip(T.DOPRI5_BETA, S.BETA)):
        assert len(a) == len(b) and all(np.float32(x) == np.float32(float(y)) for x, y in zip(a, b)), j
    for mine, spec in ((T.DOPRI5_ALPHA, S.ALPHA), (T.DOPRI5_C_ERROR, S.C_ERR), (T.DOPRI5_C_MID, S.C_MID)):
        assert all(np.float32(x) == np.float32(float(y)) for x, y in zip(mine, spec))
    ts = shifted_grid()
    assert list(T.dopri5_pending_outputs(ts, 1, ts[0] + 1e-9)) == []
    assert list(T.dopri5_pending_outputs(ts, 1, ts[3])) == [1, 2, 3]
    assert list(T.dopri5_pending_outputs(ts, 4, 1.3)) == list(range(4, 50))
    assert T.dopri5_dense_x(0.25, 0.2, 0.3) == float(np.float32((0.25 - 0.2) / (0.3 - 0.2)))
    st = T.dopri5_stage_times(0.1, 0.05)
    assert st[:4] == [np.float32(np.float32(0.1) + np.float32(a) * np.float32(0.05)) for a in (0.2, 0.3, 0.8, 8 / 9)] and st[4] == st[5] == np.float32(0.15)


def test_composed_route_follows_the_spec_on_the_cpu():
    """`transport._Dopri5` (the composed tensor-op route; the fused route needs the GPU) on an f32 CPU state takes the spec's steps and lands on its outputs;
    its counters obey NFE = 2 + 6 * attempts."""
    from dmvae_amd import transport as T
    ts = shifted_grid()
    lam, _ = lam_problem()
    y0 = torch.linspace(-1, 1, 14, dtype=torch.float32).view(2, 7) + 0.05
    want, steps, nfe = S.solve(lambda t, y: lam(t) * y, y0.double().numpy(), ts, ATOL, RTOL)
    assert min(abs(s[2] - 1) for s in steps) > 1e-3                 # no decision an f32 error ratio could flip
    fn = lambda t, y: (torch.cos(20 * t) * 6 - 1).view(-1, 1) * y
    solver = T._Dopri5(fn, y0, atol=ATOL, rtol=RTOL, fused=False, round_bf16=False)
    got = solver.solve(y0, ts, 2 ** 31 - 1)
    assert (solver.n_accepted, solver.n_rejected) == (sum(s[3] for s in steps), sum(not s[3] for s in steps))
    assert solver.nfe == nfe == 2 + 6 * len(steps)
    assert torch.equal(got[0], y0)
    assert np.abs(got.double().numpy() - want).max() < 1e-5 * np.abs(want).max()


def test_step_budget_and_non_finite_state_raise():
    from dmvae_amd import transport as T
    ts = shifted_grid()
    y0 = torch.ones(2, 3)
    with pytest.raises(RuntimeError, match="max_num_steps"):
        T._Dopri5(lambda t, y: (torch.cos(20 * t) * 6 - 1).view(-1, 1) * y, y0, atol=ATOL, rtol=RTOL, fused=False, round_bf16=False).solve(y0, ts, 1)
    bad = y0.clone()
    bad[1, 2] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        T._Dopri5(lambda t, y: -y, bad, atol=ATOL, rtol=RTOL, fused=False, round_bf16=False).solve(bad, ts, 100)
