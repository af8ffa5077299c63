"""The GVP / VP paths and noise- / score-predicting models, on the CPU: the `enable_all_paths` switch, and the host mirror `dmvae_amd.transport` against fixtures captured from the reference's own
`diffusion.transport` (tools/capture_golden_transport_paths.py: coefficient and interval tables, `sample` / `training_losses`, two `sample_sde` trajectories
per (path, prediction) pair: the eight other than Linear / velocity), and the host side of the kernel route -- `transport.model_terms`, the scalars the `_m` kernels of csrc/sampler.hip take, against the graph of
tests/transport_paths_spec.py; the new ops' argument checks that need no device."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import transport_paths_spec as S
from conftest import load_golden
from test_oracle_sampler import small_dit

pytestmark = pytest.mark.usefixtures("allow_stock")
PREDICTIONS = ["noise", "score"]
PAIRS = [("Linear", "noise"), ("Linear", "score"), ("GVP", "velocity"), ("GVP", "noise"), ("GVP", "score"), ("VP", "velocity"), ("VP", "noise"), ("VP", "score")]
EPS = {"VP": (1e-5, 1e-3), ("GVP", "velocity"): (0, 0)}          # everything else (1e-3, 1e-3)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture(path, prediction):
    return load_golden(f"transport_paths_{path.lower()}_{prediction}")


@contextlib.contextmanager
def all_paths():
    """The GVP / VP plans on for the block, the previous setting back after it."""
    from dmvae_amd.transport import enable_all_paths
    prev = enable_all_paths(True)
    try:
        yield
    finally:
        enable_all_paths(prev)


def test_gvp_and_vp_are_refused_until_the_switch_is_on():
    from dmvae_amd import transport as T
    prev = T.enable_all_paths(False)
    try:
        for path in ("GVP", "VP"):
            with pytest.raises(NotImplementedError, match="enable_all_paths"):
                T.create_transport(path, "velocity", None, 1e-3, 1e-3)
        assert T.enable_all_paths() is False                       # returns the previous setting
        assert type(T.create_transport("GVP", "noise", None, 1e-3, 1e-3).path_sampler) is T.GVPCPlan
        assert type(T.create_transport("VP", "score", None, 1e-5, 1e-3).path_sampler) is T.VPCPlan
        assert type(T.create_transport("Linear", "velocity").path_sampler) is T.ICPlan
        assert T.enable_all_paths(False) is True
        with pytest.raises(NotImplementedError):
            T.create_transport("VP", "velocity", None, 1e-5, 1e-3)
    finally:
        T.enable_all_paths(prev)


def test_running_a_script_turns_the_switch_on_and_a_bare_install_shadow_does_not(tmp_path):
    script = tmp_path / "probe_script.py"
    script.write_text("from diffusion.transport import create_transport\n"
                      "print('SCRIPT', type(create_transport('GVP', 'noise', None, 1e-3, 1e-3).path_sampler).__name__)\n")
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import run_on_mi355x as r\n"
            "r.install_shadow(None)\n"
            "import dmvae_amd.transport as T\n"
            "print('BARE', T._ALL_PATHS)\n"
            "try:\n    T.create_transport('VP', 'velocity', None, 1e-5, 1e-3)\nexcept NotImplementedError:\n    print('BARE refused')\n"
            "r.main([%r])\n"
            "print('AFTER', T._ALL_PATHS)\n") % (ROOT, str(script))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "BARE False" in out.stdout and "BARE refused" in out.stdout and "SCRIPT GVPCPlan" in out.stdout and "AFTER True" in out.stdout, out.stdout


def _transport(g):
    from dmvae_amd.transport import create_transport
    return create_transport(str(g["path"]), str(g["prediction"]), None, float(g["train_eps"]), float(g["sample_eps"]), time_dist_shift=float(g["time_dist_shift"]))


def _kw(g, tag):
    return dict(sampling_method=str(g[f"{tag}_sampling_method"]), diffusion_form=str(g[f"{tag}_diffusion_form"]), diffusion_norm=float(g[f"{tag}_diffusion_norm"]),
                last_step=str(g[f"{tag}_last_step"]), last_step_size=float(g[f"{tag}_last_step_size"]), num_steps=int(g[f"{tag}_num_steps"]))


@pytest.mark.parametrize("path,prediction", PAIRS)
def test_coefficient_and_interval_tables_equal_the_reference(path, prediction):
    from dmvae_amd.transport import ModelType
    g = fixture(path, prediction)
    with all_paths():
        tr = _transport(g)
    assert tr.model_type == {"noise": ModelType.NOISE, "score": ModelType.SCORE, "velocity": ModelType.VELOCITY}[prediction]
    assert (tr.train_eps, tr.sample_eps) == EPS.get(path, EPS.get((path, prediction), (1e-3, 1e-3)))
    ps, c = tr.path_sampler, g.t("coeffs")
    te = c[:, :1]
    full = lambda v: v.expand_as(te) if torch.is_tensor(v) else torch.full_like(te, float(v))
    alpha, d_alpha = ps.compute_alpha_t(te)
    sigma, d_sigma = ps.compute_sigma_t(te)
    got = torch.cat([te, full(alpha), full(d_alpha), full(sigma), full(d_sigma), full(ps.compute_d_alpha_alpha_ratio_t(te)),
                     full(ps.compute_drift(torch.ones_like(te), te.view(-1))[1])], dim=1)
    assert torch.equal(got, c)
    spec = torch.cat([te, full(S.alpha(te, path)[0]), full(S.alpha(te, path)[1]), full(S.sigma(te, path)[0]), full(S.sigma(te, path)[1]), full(S.ratio(te, path)),
                      full(S.drift(torch.ones_like(te), te, path)[1])], dim=1)
    assert torch.equal(spec, c)                                   # the tests' own restatement gives the reference's bits too
    rows = np.asarray(g["intervals"])
    assert len(rows) == 32
    for sbdm, sde, ev, rev, lss, t0, t1 in rows:
        got = tr.check_interval(tr.train_eps, tr.sample_eps, diffusion_form="SBDM" if sbdm else "sigma", sde=bool(sde), eval=bool(ev), reverse=bool(rev),
                                last_step_size=float(lss))
        assert got == (t0, t1), (sbdm, sde, ev, rev, lss)


@pytest.mark.parametrize("path,prediction", PAIRS)
def test_sample_training_losses_and_trajectories_vs_reference(path, prediction):
    """`sample` draws the same t and x0 (randn_like first, then rand); `training_losses` (the velocity MSE for every model type) and both `sample_sde`
    trajectories run through the host mirror on CPU tensors within tests/test_oracle_sampler.py's bar for the same mirror with a velocity model."""
    from dmvae_amd.transport import Sampler
    g = fixture(path, prediction)
    with all_paths():
        tr = _transport(g)
    m = small_dit(g["dit_seed"])
    x1, z, y = g.t("x1"), g.t("z"), torch.from_numpy(np.asarray(g["y"]))
    with torch.no_grad():
        torch.manual_seed(int(g["train_seed"]))
        t, x0, _ = tr.sample(x1)
        assert torch.equal(t, g.t("t")) and torch.equal(x0, g.t("x0"))
        torch.manual_seed(int(g["train_seed"]))
        t2, terms = tr.training_losses(m, x1, dict(y=y))
        assert torch.equal(t2, g.t("t"))
        for k in ("pred", "loss"):
            assert (terms[k] - g.t(k)).abs().max() <= 2e-6 * g.t(k).abs().max(), k
        for tag in ("euler", "heun"):
            kw, ref = _kw(g, tag), g.t(f"xs_{tag}")
            torch.manual_seed(int(g["sde_seed"]))
            xs = Sampler(tr).sample_sde(**kw)(z, m.forward, y=y)
            assert len(xs) == kw["num_steps"]
            assert (torch.stack(xs) - ref).abs().max() <= 2e-6 * ref.abs().max(), tag


@pytest.mark.parametrize("prediction", PREDICTIONS)
@pytest.mark.parametrize("tval", [1e-3, 0.5139, 0.96])
@pytest.mark.parametrize("path", ["Linear", "GVP", "VP"])
def test_model_terms_are_the_graphs_scalars(path, prediction, tval):
    """`transport.model_terms` -- what the kernel route hands the `_m` kernels -- evaluated in f32 one operation at a time (numpy: no contraction) equals the
    spec's broadcast graph bit for bit, for an f32 and a bf16 model output; the kernels do exactly this arithmetic (tests/test_gpu_transport_paths.py)."""
    from dmvae_amd import ops
    from dmvae_amd.transport import GVPCPlan, ICPlan, ModelType, VPCPlan, model_terms
    mt = {"noise": ModelType.NOISE, "score": ModelType.SCORE}[prediction]
    t = torch.tensor(tval, dtype=torch.float32)
    kind, c0, dv, nsig = model_terms({"Linear": ICPlan, "GVP": GVPCPlan, "VP": VPCPlan}[path](), mt, t.view(1, 1))
    assert kind == {"noise": ops.MODEL_NOISE, "score": ops.MODEL_SCORE}[prediction]
    g = torch.Generator().manual_seed(3)
    x, m32 = torch.randn(3, 2, 5, 7, generator=g) * 1.7, torch.randn(3, 2, 5, 7, generator=g) * 2
    f = np.float32
    for m in (m32, m32.to(torch.bfloat16)):
        want = S.velocity(prediction, m, x, torch.ones(3) * t, path)
        assert want.dtype == torch.float32
        mv, xv = m.float().numpy(), x.numpy()
        s = mv / f(nsig) if prediction == "noise" else mv
        got = f(c0) * xv + f(dv) * s
        assert got.dtype == np.float32 and np.array_equal(got, want.numpy())


def test_new_ops_reject_bad_terms_before_touching_a_device():
    from dmvae_amd import ops
    x = torch.zeros(2, 3)
    for bad in ((0, 1.0, 1.0, 1.0), (3, 1.0, 1.0, 1.0), (ops.MODEL_NOISE, 1.0, 1.0), None):
        with pytest.raises(ValueError):
            ops.model_velocity(x, x, bad)
        with pytest.raises(ValueError):
            ops.sde_euler_step_m(x, x, bad, None, 0.5, 0.5, 0.5, 0.1, 0.0, 0.0)
        with pytest.raises(ValueError):
            ops.sde_heun_predict_m(x, x, bad, 0.5, 0.5, 0.5, 0.1)
        with pytest.raises(ValueError):
            ops.sde_heun_correct_m(x, x, x, x, bad, 0.5, 0.5, 0.5, 0.05)
        with pytest.raises(ValueError):
            ops.sde_last_step_m(x, x, bad, ops.LAST_STEP_EULER, h=0.04)
    with pytest.raises(ValueError):
        ops.sde_last_step_m(x, x, (ops.MODEL_SCORE, 1.0, 1.0, 1.0), 2)


def test_library_rejects_bad_model_terms_without_a_gpu():
    """The C entry points validate before they launch: NULL pointers, n = 0 and a kind that is neither NOISE nor SCORE return -EINVAL."""
    import ctypes
    from dmvae_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok, bad = _lib.ModelTerms(1, 1.0, 1.0, -1.0), _lib.ModelTerms(0, 1.0, 1.0, -1.0)
    assert L.dmvae_model_velocity(p, p, 0, ctypes.byref(bad), p, 4, None) == -22 and b"DMVAE_MODEL_NOISE" in L.dmvae_last_error()
    assert L.dmvae_model_velocity(p, p, 0, None, p, 4, None) == -22
    assert L.dmvae_model_velocity(p, None, 0, ctypes.byref(ok), p, 4, None) == -22
    assert L.dmvae_model_velocity(p, p, 0, ctypes.byref(ok), p, 0, None) == -22
    assert L.dmvae_sde_euler_step_m(p, p, 0, ctypes.byref(bad), None, p, None, 4, 0.5, 0.5, 0.5, 0.1, 0.0, 0.0, None) == -22
    assert L.dmvae_sde_euler_step_m(p, p, 0, ctypes.byref(ok), None, None, None, 4, 0.5, 0.5, 0.5, 0.1, 0.0, 0.0, None) == -22
    assert L.dmvae_sde_heun_predict_m(p, p, 0, ctypes.byref(bad), p, p, 4, 0.5, 0.5, 0.5, 0.1, None) == -22
    assert L.dmvae_sde_heun_correct_m(p, p, p, p, 0, ctypes.byref(bad), p, 4, 0.5, 0.5, 0.5, 0.05, None) == -22
    assert L.dmvae_sde_last_step_m(p, p, 0, ctypes.byref(ok), p, 4, 2, 1.0, 0.0, 0.0, None) == -22
    assert L.dmvae_sde_last_step_m(p, p, 0, ctypes.byref(bad), p, 4, 0, 1.0, 0.0, 0.0, None) == -22


def test_library_rejects_a_bad_euler_step_without_a_gpu():
    """`dmvae_sde_euler_step` takes any n > 0 (tests/test_gpu_sampler_methods.py launches n = 5); what it still refuses before it launches: n = 0, a NULL x,
    and both outputs NULL."""
    import ctypes
    from dmvae_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.dmvae_sde_euler_step(p, p, 0, None, p, None, 0, 0.5, 0.5, 0.5, 0.1, 0.0, 0.0, None) == -22 and b"sde_euler_step" in L.dmvae_last_error()
    assert L.dmvae_sde_euler_step(None, p, 0, None, p, None, 4, 0.5, 0.5, 0.5, 0.1, 0.0, 0.0, None) == -22
    assert L.dmvae_sde_euler_step(p, p, 0, None, None, None, 4, 0.5, 0.5, 0.5, 0.1, 0.0, 0.0, None) == -22
