"""The Heun / last-step / autoguidance additions, the host side (CPU): `LightningDiT.forward_with_autoguidance`'s composition against the capture of the reference's
own method (tests/golden/autoguidance.npz, tools/capture_golden_autoguidance.py), `SamplePipeline(guidance="autoguidance")` as host logic around a stub model, the
time-vector helper of the sampler loops and the new C entry points' binding and argument validation.  The kernels are covered by tests/test_gpu_sampler_methods.py."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from test_oracle_sampler import small_dit

NEW_SYMBOLS = ("dmvae_sde_heun_perturb", "dmvae_sde_heun_predict", "dmvae_sde_heun_correct", "dmvae_sde_last_step", "dmvae_autoguidance_combine")


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def autoguidance_models(g):
    """The two models of the capture, rebuilt from the fixture's seeds: the model, and the guide with its output head perturbed the way the capture did."""
    m, guide = small_dit(g["dit_seed"]), small_dit(g["guide_seed"])
    with torch.no_grad():
        guide.final_layer.linear.weight.mul_(float(g["head_scale"]))
        guide.final_layer.linear.bias.add_(float(g["head_shift"]))
    return m, guide


def test_forward_with_autoguidance_composition_vs_reference_capture():
    """CPU f32, both models on their stock route by an explicit call (no opt-in switch): every case of the capture to 2e-6 of the tensor's largest value (the bound
    tests/test_oracle_sampler.py holds f32 restatements of the reference's modules to), and the reference's layout to the bit -- [2n, in_channels, H, W] whose two
    halves are the same tensor; outside the interval, and with the default interval, that tensor is this model's own output for the first half of the batch."""
    g = load_golden("autoguidance")
    m, guide = autoguidance_models(g)
    m.forward = m.forward_stock                              # the CPU route of `forward`, named outright
    x, y = g.t("x"), torch.from_numpy(np.asarray(g["y"]))
    scale, interval = float(g["cfg_scale"]), tuple(float(v) for v in g["interval"])
    n = x.shape[0] // 2
    inside = []
    with torch.no_grad():
        for i in range(int(g["n_cases"])):
            t, want = g.t(f"t_{i}"), g.t(f"out_{i}")
            got = m.forward_with_autoguidance(x, t, y, scale, guide.forward_stock, cfg_interval=interval)
            assert got.shape == want.shape == (2 * n, m.in_channels, *x.shape[2:])
            assert (got - want).abs().max() <= 2e-6 * want.abs().max(), i
            assert torch.equal(got, m.forward_with_autoguidance_composed(x, t, y, scale, guide.forward_stock, cfg_interval=interval))
            assert torch.equal(got[:n], got[n:])
            own = m.forward_stock(x[:n], t[:n], y[:n])[:, :m.in_channels]
            inside.append(interval[0] <= float(t[0]) <= interval[1])
            if inside[-1]:
                ag = guide.forward_stock(x[:n], t[:n], y[:n])[:, :m.in_channels]
                assert torch.equal(got[:n], ag + scale * (own - ag)) and not torch.equal(got[:n], own)
            else:
                assert torch.equal(got[:n], own)
        assert inside == [True, True, True, False, False]                                                # the edges belong to the interval
        got = m.forward_with_autoguidance(x, g.t("t_0"), y, scale, guide.forward_stock)                 # default interval: never inside
        assert (got - g.t("out_default")).abs().max() <= 2e-6 * g.t("out_default").abs().max()
        assert torch.equal(got[:n], m.forward_stock(x[:n], g.t("t_0")[:n], y[:n])[:, :m.in_channels]) and torch.equal(got[:n], got[n:])


class _StubDiT:
    """Records what the sampler hands the model; velocity = -x."""

    def __init__(self):
        self.calls = []

    def forward(self, x, t, y):
        self.calls.append(("forward", x.clone(), y.clone(), {}))
        return -x

    def forward_with_autoguidance(self, x, t, y, cfg_scale, additional_model_forward, cfg_interval=(-1e4, -1e4)):
        self.calls.append(("ag", x.clone(), y.clone(), dict(cfg_scale=cfg_scale, additional_model_forward=additional_model_forward, cfg_interval=cfg_interval)))
        half = x[: len(x) // 2]
        return -torch.cat([half, half], dim=0)


def test_sample_pipeline_autoguidance_arguments_and_doubling_on_a_stub_model():
    from dmvae_amd.sample import SamplePipeline
    with pytest.raises(ValueError, match="guide_model"):
        SamplePipeline(_StubDiT(), None, guidance="autoguidance")
    with pytest.raises(ValueError, match="guide_model"):
        SamplePipeline(_StubDiT(), None, guidance="autoguidance", cfg_scale=2.0, cfg_interval=(0.1, 0.9))
    with pytest.raises(ValueError, match="autoguidance"):
        SamplePipeline(_StubDiT(), None, guidance="auto")
    with pytest.raises(ValueError, match="cfg_interval"):
        SamplePipeline(_StubDiT(), None, guidance="autoguidance", guide_model=_StubDiT(), cfg_interval=(0.1, 0.5, 0.9))
    z, y = torch.randn(3, 4, 2, 2, generator=torch.Generator().manual_seed(1)), torch.tensor([1, 2, 3])
    kw = dict(num_sampling_steps=3, latent_mean=0.25, latent_scale=0.5, use_graph=False)

    def run(**more):
        stub = _StubDiT()
        pipe = SamplePipeline(stub, None, **kw, **more)
        torch.manual_seed(5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                    # autocast("cuda") without a GPU
            return pipe.latents(z, y), stub.calls

    guide = _StubDiT()
    tok, calls = run(guidance="autoguidance", guide_model=guide, cfg_scale=2.0, cfg_interval=(0.125, 0.875))
    assert tok.shape == (3, 4, 4) and len(calls) == 3 and all(c[0] == "ag" for c in calls)
    assert torch.equal(calls[0][1], torch.cat([z, z])) and torch.equal(calls[0][2], torch.tensor([1, 2, 3, 1, 2, 3]))
    assert calls[0][3] == dict(cfg_scale=2.0, additional_model_forward=guide.forward, cfg_interval=(0.125, 0.875))
    fn = lambda x, t, y: -x                                                                             # a bare callable is its own forward
    _, calls = run(guidance="autoguidance", guide_model=fn)
    assert calls[0][3] == dict(cfg_scale=1.0, additional_model_forward=fn, cfg_interval=(-1e4, -1e4))
    base, calls = run()                                                                                  # the unguided path: as before, guide_model ignored
    assert all(c[0] == "forward" and c[1].shape[0] == 3 for c in calls)
    assert torch.equal(run(guide_model=guide)[0], base)


def test_time_vector_is_the_reference_expression():
    """`_time_vector(n, t, like)` == `th.ones(n).to(x) * t` and `_time_vector(n, t, device=)` == `th.ones(n).to(device) * t` on the CPU: value, dtype, bits."""
    from dmvae_amd.transport import _time_vector
    t = torch.linspace(0, 0.96, 7)[3]
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        x = torch.zeros(5, 2, dtype=dtype)
        want = torch.ones(5).to(x) * t
        got = _time_vector(5, t, x)
        assert got.dtype == want.dtype and torch.equal(got, want)
    got = _time_vector(4, t + 0.5 * t, device="cpu")
    assert got.dtype == torch.float32 and torch.equal(got, torch.ones(4) * (t + 0.5 * t))


def test_new_entry_points_are_bound_and_validate_without_gpu(lib):
    from dmvae_amd import _lib, ops
    assert lib.dmvae_abi_version() == 9                        # new entry points are a compatible extension
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    bufs = [ctypes.create_string_buffer(64) for _ in range(3)]
    p, q, r = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    assert lib.dmvae_sde_heun_perturb(None, p, q, 4, 1.0, 1.0, None) == -22 and b"sde_heun_perturb" in lib.dmvae_last_error()
    assert lib.dmvae_sde_heun_perturb(p, q, r, 0, 1.0, 1.0, None) == -22
    assert lib.dmvae_sde_heun_predict(p, None, 0, q, r, 4, 0.5, 0.5, 0.5, 0.1, None) == -22 and b"sde_heun_predict" in lib.dmvae_last_error()
    assert lib.dmvae_sde_heun_correct(p, q, r, None, 1, p, 4, 0.5, 0.5, 0.5, 0.05, None) == -22 and b"sde_heun_correct" in lib.dmvae_last_error()
    assert lib.dmvae_sde_last_step(p, q, 0, None, 4, 0, 1.0, 0.0, 0.5, 0.5, 0.0, None) == -22 and b"sde_last_step" in lib.dmvae_last_error()
    assert lib.dmvae_sde_last_step(p, q, 0, r, 4, 2, 1.0, 0.0, 0.5, 0.5, 0.0, None) == -22 and b"mode" in lib.dmvae_last_error()
    t = ctypes.cast(ctypes.create_string_buffer(4), ctypes.c_void_p)
    assert lib.dmvae_autoguidance_combine(p, 2, q, 2, 0, r, 1, 4, 2, 2.5, None, 0.0, 1.0, None) == -22 and b"NULL" in lib.dmvae_last_error()
    assert lib.dmvae_autoguidance_combine(p, 2, q, 2, 0, p, 1, 4, 2, 2.5, t, 0.0, 1.0, None) == -22 and b"alias" in lib.dmvae_last_error()
    for k in (0, 3):                                           # no channel, more than either output has
        assert lib.dmvae_autoguidance_combine(p, 2, q, 4, 0, r, 1, 4, k, 2.5, t, 0.0, 1.0, None) == -22 and b"k <=" in lib.dmvae_last_error()
    assert lib.dmvae_autoguidance_combine(p, 2, q, 2, 0, r, 0, 4, 2, 2.5, t, 0.0, 1.0, None) == -22
    x = torch.zeros(2, 3, 2, 2)
    for call in (lambda: ops.sde_heun_perturb(x, x, 1.0, 1.0), lambda: ops.sde_heun_predict(x, x, 0.5, 0.5, 0.5, 0.1),
                 lambda: ops.sde_heun_correct(x, x, x, x, 0.5, 0.5, 0.5, 0.05), lambda: ops.sde_last_step(x, x, ops.LAST_STEP_EULER, h=0.04),
                 lambda: ops.autoguidance_combine(x, x, 3, 2.5, torch.zeros(2))):
        with pytest.raises(_lib.DmvaeHipError):                # no CPU path: a CPU tensor is an error, never a fall-back
            call()
