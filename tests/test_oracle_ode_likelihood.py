"""The likelihood sampler (`Sampler.sample_ode_likelihood`, the reference's transport.py:402-459) on the CPU: the float64 tuple-state restatement of
tests/dopri5_tuple_spec.py (torchdiffeq's mixed norm) checked against a flat-norm solve and the closed-form likelihood of Gaussian data, the composed
tuple-state route of `dmvae_amd.transport._Dopri5` against it, and the drift's Hutchinson term against a dense Jacobian."""
import numpy as np
import pytest
import torch

import dopri5_spec as S
import dopri5_tuple_spec as TS

ATOL, RTOL = 1e-6, 1e-3


def _grid(num_steps=50):
    from dmvae_amd.transport import ode
    return ode(None, t0=0, t1=1, sampler_type="dopri5", num_steps=num_steps, atol=ATOL, rtol=RTOL).t.double().tolist()


def _two_part_problem(nx=400):
    """x' = -x on 400 elements (smooth, small error) and one scalar l' = 6 cos(20 t) (fast, large error): the flat RMS divides the scalar's error by
    sqrt(401), the mixed norm does not."""
    def f(t, y):
        return np.concatenate([-y[:nx], [6 * np.cos(20 * t)]])
    y0 = np.concatenate([np.linspace(0.5, 1.5, nx), [0.0]])
    return f, y0, [(0, nx), (nx, nx + 1)]


def test_mixed_norm_changes_the_step_sequence():
    f, y0, parts = _two_part_problem()
    ts = _grid()
    _, mixed, nfe_m = TS.solve(f, y0, ts, ATOL, RTOL, parts=parts)
    _, flat, nfe_f = TS.solve(f, y0, ts, ATOL, RTOL)
    _, flat_ref, nfe_r = S.solve(f, y0, ts, ATOL, RTOL)
    assert flat == flat_ref and nfe_f == nfe_r                  # parts=None is dopri5_spec.solve itself
    assert len(mixed) > len(flat) and nfe_m > nfe_f, (len(mixed), len(flat))
    # the mixed norm is the larger one here: every step it accepts has the scalar part's RMS within tolerance
    assert TS.mixed_norm(parts)(np.array([0.0] * 400 + [1.0])) == 1.0 and S.rms(np.array([0.0] * 400 + [1.0])) < 0.05


@pytest.mark.parametrize("s", [0.5, 1.7])
def test_spec_reproduces_the_gaussian_closed_form(s):
    d, b = 12, 3
    x = np.random.default_rng(3).standard_normal((b, d)) * s
    y0 = np.concatenate([x.ravel(), np.zeros(b)])
    out, steps, _ = TS.solve(TS.gaussian_likelihood_drift(s, d, b), y0, _grid(), 1e-9, 1e-9, parts=[(0, b * d), (b * d, b * d + b)])
    z, dlogp = out[-1][:b * d].reshape(b, d), out[-1][b * d:]
    want_logp, want_z = TS.gaussian_logp(x, s)
    logp = (-d / 2 * np.log(2 * np.pi) - (z ** 2).sum(1) / 2) - dlogp        # Transport.prior_logp(z) - delta_logp
    assert np.abs(logp - want_logp).max() < 1e-7 * np.abs(want_logp).max()
    assert np.abs(z - want_z).max() < 1e-7 * np.abs(want_z).max()
    assert all(st[3] for st in steps[-3:])


def test_composed_tuple_route_follows_the_spec():
    """`_Dopri5` on a flat CPU f32 buffer with parts (its composed route: tensor ops only) takes the float64 spec's steps on the Gaussian problem and lands
    within f32 rounding of the spec's result."""
    from dmvae_amd.transport import _Dopri5
    s, d, b = 0.6, 48, 4
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((b, d)) * s).float()
    nx = b * d
    y0 = torch.cat([x.reshape(-1), torch.zeros(b)])
    parts = [(0, nx), (nx, nx + b)]

    def fn_into(t, y, out):
        a = float(TS.gaussian_rate(1 - t[0].double().item(), s))
        out[:nx].copy_(-a * y[:nx])
        out[nx:].fill_(d * a)

    ts = _grid()
    solver = _Dopri5(None, y0, atol=ATOL, rtol=RTOL, fused=False, round_bf16=False, parts=parts, batch=b, fn_into=fn_into)
    got = solver.solve(y0, ts, 2 ** 31 - 1)
    want, steps, nfe = TS.solve(TS.gaussian_likelihood_drift(s, d, b), y0.double().numpy(), ts, ATOL, RTOL, parts=parts)
    assert min(abs(st[2] - 1) for st in steps) > 1e-3
    assert (solver.nfe, solver.n_accepted, solver.n_rejected) == (nfe, sum(st[3] for st in steps), sum(not st[3] for st in steps))
    assert got.shape == (50, nx + b)
    assert np.abs(got.double().numpy() - want).max() < 2e-5 * np.abs(want).max()


def test_likelihood_drift_is_hutchinson_with_one_model_call():
    """The drift the sampler hands the solver: (-v(x, 1 - t), eps^T J eps) with eps the reference's own draw (th.randint on x's device) and J the dense
    Jacobian of a small non-diagonal nonlinear model; the model is called once per evaluation (the reference's second call is dropped: it would return the
    same values)."""
    from dmvae_amd.transport import Sampler, create_transport
    g = torch.Generator().manual_seed(0)
    w = torch.randn(6, 6, generator=g, dtype=torch.float64) * 0.5
    calls = []

    def model(x, t):
        calls.append(1)
        return torch.tanh(x @ w.to(x.dtype) + t.view(-1, 1)) * x.flip(1)

    fn = Sampler(create_transport()).sample_ode_likelihood()
    drift = fn.ode.drift
    x = torch.randn(3, 6, generator=g)
    t = torch.full((3,), 0.3)
    torch.manual_seed(7)
    neg_v, lg = drift((x, torch.zeros(3)), t, model)
    assert len(calls) == 1
    torch.manual_seed(7)
    eps = torch.randint(2, x.size(), dtype=torch.float) * 2 - 1
    assert torch.equal(neg_v, -model(x, torch.ones_like(t) * (1 - t)))
    for i in range(3):
        jac = torch.autograd.functional.jacobian(lambda r: model(r.view(1, 6), torch.full((1,), 0.7, dtype=torch.float64)).view(6), x[i].double())
        want = (eps[i].double() @ jac @ eps[i].double()).item()
        assert abs(lg[i].item() - want) < 1e-5 * max(1.0, abs(want))
    assert x.grad is None and not x.requires_grad


def test_cpu_tuple_state_without_torchdiffeq_raises():
    from dmvae_amd.transport import Sampler, create_transport
    try:
        import torchdiffeq  # noqa: F401
        have = True
    except ImportError:
        have = False
    fn = Sampler(create_transport()).sample_ode_likelihood(sampling_method="euler", num_steps=3)
    model = lambda x, t: x * 0.5
    if have:
        logp, z = fn(torch.randn(2, 4), model)
        assert logp.shape == (2,) and z.shape == (2, 4)
    else:
        with pytest.raises(NotImplementedError):
            fn(torch.randn(2, 4), model)
        with pytest.raises(NotImplementedError):
            Sampler(create_transport()).sample_ode_likelihood()(torch.randn(2, 4), model)
