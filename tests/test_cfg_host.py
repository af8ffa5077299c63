"""Classifier-free guided sampling, the host side (CPU): `LightningDiT.forward_with_cfg`'s dispatch leaves the CPU route the reference's composition, the
label / latent doubling of `dmvae_amd.sample` as pure host logic around a stub model, `dmvae_cfg_combine`'s argument validation and the single-process form
of `dist.all_gather_into`.  The kernel route is covered by tests/test_gpu_cfg.py."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from test_oracle_sampler import small_dit


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_forward_with_cfg_on_cpu_is_the_reference_composition(allow_stock):
    """The new dispatch on CPU tensors: the six-step guided Euler-Maruyama trajectory captured from the reference's own forward_with_cfg (the bound of
    tests/test_oracle_sampler.py::test_sde_sampler_with_cfg_vs_reference), and bit-equality with the composition kept as `forward_with_cfg_composed`,
    interval gate included."""
    from dmvae_amd.transport import Sampler, create_transport
    g = load_golden("sampler_euler_cfg")
    m = small_dit(g["dit_seed"])
    z, y = g.t("z"), torch.from_numpy(np.asarray(g["y"]))
    fn = Sampler(create_transport()).sample_sde(sampling_method="Euler", diffusion_form="sigma", last_step="Mean", last_step_size=0.04, num_steps=int(g["num_steps"]))
    with torch.no_grad():
        torch.manual_seed(int(g["seed"]))
        xs = fn(z, m.forward_with_cfg, y=y, cfg_scale=float(g["cfg_scale"]), standard_cfg=True)
        assert (torch.stack(xs) - g.t("xs")).abs().max() <= 2e-6 * g.t("xs").abs().max()
        t = torch.full((z.shape[0],), 0.3)
        for kw in (dict(), dict(standard_cfg=True), dict(cfg_interval=True, cfg_interval_start=0.5), dict(cfg_interval=True, cfg_interval_start=0.1, standard_cfg=True)):
            assert torch.equal(m.forward_with_cfg(z, t, y, 2.5, **kw), m.forward_with_cfg_composed(z, t, y, 2.5, **kw)), kw
        gated = m.forward_with_cfg(z, t, y, 2.5, cfg_interval=True, cfg_interval_start=0.5)
        n = z.shape[0] // 2
        assert torch.equal(gated[:n, :3], m.forward(torch.cat([z[:n], z[:n]]), t, y)[:n, :3])           # below the start: the conditional output


class _StubDiT:
    """Records what the sampler hands the model; velocity = -x (any smooth field does)."""

    class _Y:
        num_classes = 10

    def __init__(self):
        self.y_embedder, self.calls = self._Y(), []

    def forward(self, x, t, y):
        self.calls.append(("forward", x.clone(), y.clone(), {}))
        return -x

    def forward_with_cfg(self, x, t, y, cfg_scale, cfg_interval=None, cfg_interval_start=None, standard_cfg=False):
        self.calls.append(("cfg", x.clone(), y.clone(), dict(cfg_scale=cfg_scale, cfg_interval=cfg_interval, cfg_interval_start=cfg_interval_start,
                                                               standard_cfg=standard_cfg)))
        half = x[: len(x) // 2]
        return -torch.cat([half, half], dim=0)


def test_cfg_inputs_and_guided_sample_are_the_reference_doubling():
    from dmvae_amd.sample import cfg_inputs, guided_sample
    z, y = torch.randn(3, 4, 2, 2, generator=torch.Generator().manual_seed(0)), torch.tensor([7, 0, 3])
    zz, yy = cfg_inputs(z, y, 10)
    assert torch.equal(zz, torch.cat([z, z])) and torch.equal(yy, torch.tensor([7, 0, 3, 10, 10, 10])) and yy.dtype == y.dtype
    seen = {}

    def sample_fn(x, model, **kw):
        seen.update(x=x, model=model, kw=kw)
        return [x * 0, x + torch.arange(6.0).view(6, 1, 1, 1)]

    out = guided_sample(sample_fn, lambda a, b: ("fn", a.shape[0], b.shape[0]), z, y, 10, cfg_scale=2.5, standard_cfg=True)
    assert torch.equal(out, z + torch.arange(3.0).view(3, 1, 1, 1))                                      # the last state's first half
    assert seen["model"] == ("fn", 6, 6) and torch.equal(seen["x"], zz) and torch.equal(seen["kw"]["y"], yy)
    assert seen["kw"]["cfg_scale"] == 2.5 and seen["kw"]["standard_cfg"] is True


def test_sample_pipeline_guidance_keyword_on_a_stub_model():
    """`guidance="cfg"`: the sampler sees [z | z], [y | null] and forward_with_cfg's keywords, n samples come back; the default ignores cfg_scale as before."""
    from dmvae_amd.sample import SamplePipeline
    z, y = torch.randn(3, 4, 2, 2, generator=torch.Generator().manual_seed(1)), torch.tensor([1, 2, 3])
    kw = dict(num_sampling_steps=3, latent_mean=0.25, latent_scale=0.5, use_graph=False)

    def run(**more):
        stub = _StubDiT()
        pipe = SamplePipeline(stub, None, **kw, **more)
        torch.manual_seed(5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                    # autocast("cuda") without a GPU
            return pipe.latents(z, y), stub.calls

    tok, calls = run(guidance="cfg", cfg_scale=2.5)
    assert tok.shape == (3, 4, 4) and len(calls) == 3 and all(c[0] == "cfg" for c in calls)
    assert torch.equal(calls[0][1], torch.cat([z, z])) and torch.equal(calls[0][2], torch.tensor([1, 2, 3, 10, 10, 10]))
    assert calls[0][3] == dict(cfg_scale=2.5, cfg_interval=None, cfg_interval_start=None, standard_cfg=True)
    _, calls = run(guidance="cfg", cfg_scale=2.5, standard_cfg=False, cfg_interval_start=0.125)
    assert calls[0][3] == dict(cfg_scale=2.5, cfg_interval=True, cfg_interval_start=0.125, standard_cfg=False)
    base, calls = run()
    assert all(c[0] == "forward" and c[1].shape[0] == 3 for c in calls)
    for more in (dict(cfg_scale=2.5), dict(guidance="cfg", cfg_scale=1.0)):                              # ignored / the unguided path
        tok2, calls = run(**more)
        assert torch.equal(tok2, base) and all(c[0] == "forward" and c[1].shape[0] == 3 for c in calls)
    _, calls = run(guidance="cfg", cfg_scale=2.5, mode="ODE", sampling_method="euler")
    assert calls and all(c[0] == "cfg" and c[1].shape[0] == 6 for c in calls)
    with pytest.raises(ValueError):
        SamplePipeline(_StubDiT(), None, guidance="autoguidance")


def test_cfg_combine_argument_validation_without_gpu(lib):
    buf, buf2 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf2, ctypes.c_void_p)
    assert lib.dmvae_cfg_combine(None, 1, q, 1, 2, 4, 2, 2.5, None, 0.0, None) == -22 and b"cfg_combine" in lib.dmvae_last_error()
    assert lib.dmvae_cfg_combine(p, 1, None, 1, 2, 4, 2, 2.5, None, 0.0, None) == -22 and b"NULL" in lib.dmvae_last_error()
    assert lib.dmvae_cfg_combine(p, 1, p, 1, 2, 4, 2, 2.5, None, 0.0, None) == -22 and b"alias" in lib.dmvae_last_error()
    for n in (0, -3):
        assert lib.dmvae_cfg_combine(p, 0, q, n, 2, 4, 2, 2.5, None, 0.0, None) == -22 and b"n > 0" in lib.dmvae_last_error()
    assert lib.dmvae_cfg_combine(p, 0, q, 1, 2, 4, -1, 2.5, None, 0.0, None) == -22 and b"k >= 0" in lib.dmvae_last_error()
    assert lib.dmvae_cfg_combine(p, 0, q, 1, 0, 4, 0, 2.5, None, 0.0, None) == -22
    assert lib.dmvae_abi_version() == 9                        # a new entry point is a compatible extension


def test_ops_cfg_combine_refuses_cpu_tensors():
    from dmvae_amd import _lib, ops
    with pytest.raises(_lib.DmvaeHipError):
        ops.cfg_combine(torch.zeros(2, 3, 2, 2), 3, 2.5)


def test_all_gather_into_is_a_copy_without_a_process_group():
    from dmvae_amd import dist
    t = torch.arange(12.0).view(3, 4)
    out = torch.zeros(3 * dist.get_world_size(), 4)
    assert dist.all_gather_into(out, t) is out and torch.equal(out, t)
