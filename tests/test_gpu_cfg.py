"""Classifier-free guided sampling on the MI355X (-m gpu): the guidance kernel (csrc/sampler.hip::cfg_combine_kernel) bit-exact against the reference's
expression evaluated by PyTorch on the CPU, `LightningDiT.forward_with_cfg` on the kernels and its graph against the tensor-op composition, the guided
sampler against the trajectory captured from the reference, `SamplePipeline(guidance="cfg")` and `DiffusionTrainer.sample`."""
import copy
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from test_oracle_sampler import small_dit

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def composed_cfg(fwd, in_channels):
    """The reference's forward_with_cfg (lightningdit.py:423-447) as tensor ops over `fwd`: the yardstick (the method itself now dispatches)."""
    def f(x, t, y, cfg_scale, cfg_interval=None, cfg_interval_start=None, standard_cfg=False):
        half = x[: len(x) // 2]
        out = fwd(torch.cat([half, half], dim=0), t, y)
        k = in_channels if standard_cfg else 3
        eps, rest = out[:, :k], out[:, k:]
        cond, uncond = torch.split(eps, len(eps) // 2, dim=0)
        half_eps = uncond + cfg_scale * (cond - uncond)
        if cfg_interval is True and t[0] < cfg_interval_start:
            half_eps = cond
        return torch.cat([torch.cat([half_eps, half_eps], dim=0), rest], dim=1)
    return f


def _ref_combine(out, k, scale, t, start):
    """lightningdit.py:434-447 on the model's output, evaluated where it is called (the CPU), in the tensor's own dtype."""
    eps, rest = out[:, :k], out[:, k:]
    cond, uncond = torch.split(eps, len(eps) // 2, dim=0)
    half_eps = uncond + scale * (cond - uncond)
    if t is not None and t[0] < start:
        half_eps = cond
    return torch.cat([torch.cat([half_eps, half_eps], dim=0), rest], dim=1)


@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("n", [1, 2, 25])
@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 16, 16), (5, 1, 7)])
def test_cfg_combine_kernel_bit_exact(dtype, n, shape):
    """ops.cfg_combine == the reference's expression on the CPU, torch.equal, no tolerance: bf16 and f32, quads and the scalar tail ((5, 7)), k in {0, 3, C},
    the interval gate off / below / at / above the start; +-0, a bf16 subnormal, +-inf among the inputs, one NaN lane checked to come out NaN."""
    from dmvae_amd import ops
    c, h, w = shape
    g = torch.Generator().manual_seed(1000 * n + c)
    out = (torch.randn(2 * n, c, h, w, generator=g) * 2).to(dtype)
    sub = 2.0 ** -130                                                     # a bf16 (and f32) subnormal
    for ch in (0, c - 1):
        out[0, ch, 0, :7] = torch.tensor([0.0, -0.0, sub, float("inf"), 0.5, float("nan"), 3.0]).to(dtype)
        out[n, ch, 0, :7] = torch.tensor([-0.0, -0.0, -3 * sub, 1.0, float("-inf"), 1.0, sub]).to(dtype)
    dev_in = out.to(DEV)
    start = 0.5
    gates = [None, torch.tensor([0.25, 0.9]), torch.tensor([0.5, 0.1]), torch.tensor([0.75, 0.1])]      # off, below, at, above
    for i, k in enumerate((0, 3, c)):
        for j, t in enumerate(gates):
            scale = (1.5, 2.5, 4.0)[(i + j) % 3]                          # exactly representable in bf16
            want = _ref_combine(out, k, scale, t, start)
            got = ops.cfg_combine(dev_in, k, scale, None if t is None else t.to(DEV), start).cpu()
            assert got.dtype == dtype and got.shape == want.shape
            nan = torch.isnan(want)
            assert bool(nan[0, 0, 0, 5]) and torch.equal(torch.isnan(got), nan), (k, j)
            assert torch.equal(got[~nan], want[~nan]), (k, j)
            assert torch.equal(torch.signbit(got[~nan].float()), torch.signbit(want[~nan].float())), (k, j)      # -0 stays -0
    assert torch.equal(dev_in.cpu()[~torch.isnan(out)], out[~torch.isnan(out)])                         # the input is not written
    # k beyond C is clamped; an f64 t is converted on the device
    assert torch.equal(torch.nan_to_num(ops.cfg_combine(dev_in, c + 5, 2.5).float()), torch.nan_to_num(ops.cfg_combine(dev_in, c, 2.5).float()))
    t64 = torch.tensor([0.25], dtype=torch.float64, device=DEV)
    assert torch.equal(torch.nan_to_num(ops.cfg_combine(dev_in, c, 2.5, t64, start).float()), torch.nan_to_num(_ref_combine(out, c, 2.5, t64.cpu(), start).float()).to(DEV))


def test_cfg_combine_validates_inputs():
    from dmvae_amd import ops
    x = torch.zeros(4, 3, 2, 2, device=DEV)
    with pytest.raises(ValueError):
        ops.cfg_combine(x[:3], 3, 2.5)                                    # odd batch
    with pytest.raises(ValueError):
        ops.cfg_combine(x.transpose(2, 3), 3, 2.5)                        # not contiguous
    with pytest.raises(TypeError):
        ops.cfg_combine(x.double(), 3, 2.5)
    with pytest.raises(ValueError):
        ops.cfg_combine(x, 3, 2.5, out=x)                                 # aliasing
    with pytest.raises(ValueError):
        ops.cfg_combine(x, -1, 2.5)
    with pytest.raises(ValueError):
        ops.cfg_combine(x, 3, 2.5, t=torch.zeros(1))                      # t on the CPU
    with pytest.raises(ValueError):
        ops.cfg_combine(x, 3, 2.5, out=torch.zeros(4, 3, 2, 3, device=DEV))


def _cfg_case(n=3, seed=3):
    g = load_golden("sampler_euler_cfg")
    m = small_dit(g["dit_seed"]).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(seed)

    def mk():
        x = torch.randn(2 * n, 8, 8, 8, device=DEV, generator=gen)
        t = torch.rand(1, device=DEV, generator=gen).clamp(0.3, 0.7).expand(2 * n).contiguous()
        y = torch.cat([torch.randint(0, 10, (n,), device=DEV, generator=gen), torch.full((n,), 10, device=DEV)])
        return x, t, y
    return m, mk


def test_forward_with_cfg_route_equals_the_composition_bit_for_bit():
    """The fixture's small DiT under autocast(bf16): forward_with_cfg (2n forward + one guidance kernel) == the ten-line composition over m.forward, for
    standard_cfg True / False and the interval gate closed / open."""
    m, mk = _cfg_case()
    ref = composed_cfg(m.forward, m.in_channels)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        for it in range(2):
            x, t, y = mk()
            for kw in (dict(), dict(standard_cfg=True), dict(standard_cfg=True, cfg_interval=True, cfg_interval_start=0.9),
                       dict(cfg_interval=True, cfg_interval_start=0.9), dict(standard_cfg=True, cfg_interval=True, cfg_interval_start=0.1)):
                want = ref(x, t, y, 2.5, **kw)
                got = m.forward_with_cfg(x, t, y, 2.5, **kw)
                assert got.dtype == BF and torch.equal(got, want), kw
                assert torch.equal(m.forward_with_cfg_composed(x, t, y, 2.5, **kw), want)
        guided, gated = m.forward_with_cfg(x, t, y, 2.5, standard_cfg=True), m.forward_with_cfg(x, t, y, 2.5, standard_cfg=True, cfg_interval=True, cfg_interval_start=0.9)
        assert not torch.equal(guided, gated) and guided.float().abs().max() > 0                      # guidance does something on this model
        assert m._takes_inference_route(x)
    with torch.autocast("cuda", dtype=BF):                                # a gradient wanted: the composition over the training route, as before
        assert not m._takes_inference_route(x)
    assert not m._takes_inference_route(x)                                # outside autocast: not the kernels' call


def test_graphed_guided_forward_replays_bit_exactly_and_captures_the_gate():
    """lightningdit_fast.GraphedInferenceCfg == the ungraphed guided route for fresh inputs; other shapes and other guidance settings are refused; with
    cfg_interval=True the graph CAPTURES (the gate is compared on the device) and follows the replayed t on both sides of the start."""
    from dmvae_amd.models import lightningdit_fast as fast
    m, mk = _cfg_case(seed=4)
    m = m.eval().requires_grad_(False)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        gi = fast.GraphedInferenceCfg(m, *mk(), cfg_scale=2.5, standard_cfg=True)
        for _ in range(3):
            x, t, y = mk()
            want = m.forward_with_cfg(x, t, y, 2.5, standard_cfg=True).clone()
            assert torch.equal(gi(x, t, y, cfg_scale=2.5, standard_cfg=True), want)
            assert torch.equal(gi(x, t, y), want)
        with pytest.raises(AssertionError):
            gi(x[:4], t[:4], y[:4])
        with pytest.raises(AssertionError):
            gi(x, t, y, cfg_scale=4.0, standard_cfg=True)
        with pytest.raises(AssertionError):
            gi(x, t, y, cfg_scale=2.5, standard_cfg=False)
        with pytest.raises(AssertionError):
            gi(x, t, y, cfg_scale=2.5, standard_cfg=True, cfg_interval=True, cfg_interval_start=0.5)
        assert gi.matches(x, t, y, 2.5, 8, None) and not gi.matches(x, t, y, 2.5, 3, None) and not gi.matches(x, t, y, 2.5, 8, 0.5)
        gg = fast.GraphedInferenceCfg(m, *mk(), cfg_scale=4.0, cfg_interval=True, cfg_interval_start=0.5)       # the capture itself is the point
        outs = []
        for tv in (0.2, 0.5, 0.8):
            x, _, y = mk()
            t = torch.full((x.shape[0],), tv, device=DEV)
            want = m.forward_with_cfg(x, t, y, 4.0, cfg_interval=True, cfg_interval_start=0.5).clone()
            got = gg(x, t, y, cfg_scale=4.0, cfg_interval=True, cfg_interval_start=0.5)
            assert torch.equal(got, want), tv
            n = x.shape[0] // 2
            outs.append(torch.equal(got[:n, :3], m.forward(torch.cat([x[:n], x[:n]]), t, y)[:n, :3]))   # the conditional output itself?
        assert outs == [True, False, False]


def test_guided_sampler_on_hip_dit_vs_reference_trajectory():
    """`sampler_euler_cfg` (the reference's own forward_with_cfg, cfg_scale 2.5, standard_cfg) on the GPU: the criterion of
    test_gpu_sampler.py::test_sampler_on_hip_dit_vs_reference_trajectory unchanged -- as close to the f32 capture as guidance composed over the stock modules
    under autocast, x 2, floor 2e-2 -- and bit-equality with the sampler composed of tensor ops."""
    from dmvae_amd import transport as T
    g = load_golden("sampler_euler_cfg")
    m = small_dit(g["dit_seed"]).to(DEV)
    z, y, ref = g.t("z").to(DEV), torch.from_numpy(np.asarray(g["y"])).to(DEV), g.t("xs")
    sampler = T.Sampler(T.create_transport())

    def run(model_fn, fused=True):
        fn = sampler.sample_sde(sampling_method="Euler", diffusion_form="sigma", last_step="Mean", last_step_size=0.04, num_steps=int(g["num_steps"]))
        T.FUSED_STATE_UPDATE = fused
        try:
            torch.manual_seed(int(g["seed"]))
            with torch.no_grad(), torch.autocast("cuda", dtype=BF):
                return torch.stack(fn(z, model_fn, y=y, cfg_scale=float(g["cfg_scale"]), standard_cfg=True)).float().cpu()
        finally:
            T.FUSED_STATE_UPDATE = True

    hip = run(m.forward_with_cfg)
    stock = run(composed_cfg(m.forward_stock, m.in_channels))
    e_hip, e_stock = rel_err(hip, ref), rel_err(stock, ref)
    print(f"guided sampler: rel err to the reference's capture -- HIP {e_hip:.3e}, stock autocast {e_stock:.3e}; last state {rel_err(hip[-1], ref[-1]):.3e} / "
          f"{rel_err(stock[-1], ref[-1]):.3e}")
    assert e_hip < max(2 * e_stock, 2e-2), (e_hip, e_stock)
    assert rel_err(hip[-1], ref[-1]) < max(2 * rel_err(stock[-1], ref[-1]), 2e-2)
    assert torch.equal(hip, run(m.forward_with_cfg, fused=False))


def _pipeline_dit():
    from dmvae_amd.models.lightningdit import LightningDiT
    torch.manual_seed(8)
    dit = LightningDiT(input_size=16, patch_size=1, in_channels=32, hidden_size=144, depth=3, num_heads=2, num_classes=10).to(DEV).eval().requires_grad_(False)
    with torch.no_grad():
        for blk in dit.blocks:
            blk.adaLN_modulation[1].weight.normal_(0, 0.02)
        dit.final_layer.linear.weight.normal_(0, 0.05)
    return dit


def test_sample_pipeline_with_guidance():
    from dmvae_amd.models import lightningdit_fast as fast
    from dmvae_amd.sample import SamplePipeline, dit_output_to_tokens
    from dmvae_amd.transport import Sampler, create_transport
    dit = _pipeline_dit()
    g = torch.Generator(device=DEV).manual_seed(1)
    z, y = torch.randn(5, 32, 16, 16, device=DEV, generator=g), torch.tensor([0, 3, 5, 7, 9], device=DEV)
    kw = dict(num_sampling_steps=7, latent_mean=0.0685, latent_scale=0.1763)
    outs = []
    for use_graph in (True, False):
        pipe = SamplePipeline(dit, None, guidance="cfg", cfg_scale=2.5, use_graph=use_graph, **kw)
        torch.manual_seed(77)
        outs.append(pipe.latents(z, y))
        assert isinstance(pipe._graphed, fast.GraphedInferenceCfg) == use_graph
    assert outs[0].shape == (5, 256, 32) and torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    # the sampler driven by hand: [z | z], [y | null], the first half of the last state
    fn = Sampler(create_transport("Linear", "velocity", None, 0.0, 0.0, time_dist_shift=1.0)).sample_sde(
        sampling_method="Euler", diffusion_form="sigma", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04, num_steps=7)
    torch.manual_seed(77)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        last = fn(torch.cat([z, z]), dit.forward_with_cfg, y=torch.cat([y, torch.full_like(y, 10)]), cfg_scale=2.5, standard_cfg=True)[-1]
    assert torch.equal(outs[0], dit_output_to_tokens(last.chunk(2)[0].float(), 0.0685, 0.1763))
    # the default still ignores cfg_scale (sample_50k.py:120); guidance with scale 1 is the unguided path
    base = []
    for more in (dict(cfg_scale=1.0), dict(cfg_scale=2.5), dict(guidance="cfg", cfg_scale=1.0)):
        pipe = SamplePipeline(dit, None, **kw, **more)
        torch.manual_seed(77)
        base.append(pipe.latents(z, y))
        assert type(pipe._graphed) is fast.GraphedInference
    assert torch.equal(base[0], base[1]) and torch.equal(base[0], base[2]) and not torch.equal(base[0], outs[0])
    # ODE mode on a fixed grid runs guided too
    ode = []
    for use_graph in (True, False):
        pipe = SamplePipeline(dit, None, guidance="cfg", cfg_scale=2.5, mode="ODE", sampling_method="euler", use_graph=use_graph, **kw)
        ode.append(pipe.latents(z, y))
    assert ode[0].shape == (5, 256, 32) and torch.isfinite(ode[0]).all() and torch.equal(ode[0], ode[1])
    unguided = SamplePipeline(dit, None, mode="ODE", sampling_method="euler", **kw).latents(z, y)
    assert not torch.equal(ode[0], unguided)


def _trainer_parts():
    from dmvae_amd.models.lightningdit import LightningDiT
    from dmvae_amd.models.vae import VAE
    torch.manual_seed(6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = VAE(z_channels=32, model_size="base", encoder_kwargs=dict(embed_dim=256, depth=1, num_heads=4)).to(DEV).eval()
    kw = dict(input_size=16, patch_size=1, in_channels=32, hidden_size=192, depth=2, num_heads=3, num_classes=10)
    dit = LightningDiT(**kw).to(DEV)
    with torch.no_grad():
        for blk in dit.blocks:
            blk.adaLN_modulation[1].weight.normal_(0, 0.02)
        dit.final_layer.linear.weight.normal_(0, 0.05)
    return vae, dit, kw


def test_diffusion_trainer_sample():
    """DiffusionTrainer.sample (train_diffusion.py:242-258,335-359): leaves training untouched -- step, step, sample, step, step == four steps, bit for bit in
    weights, EMA and optimiser state --, equals the sampler run by hand on a model loaded from ema_state_dict(), follows the EMA as it moves, takes the unguided
    branch at cfg_scale 1, restores nothing because it changes nothing of the training model (mode included); one default dopri5 call finishes."""
    from dmvae_amd.models.lightningdit import LightningDiT
    from dmvae_amd.sample import dit_output_to_tokens
    from dmvae_amd.train import DiffusionTrainer
    from dmvae_amd.transport import Sampler
    vae, dit, dkw = _trainer_parts()
    dit_b = copy.deepcopy(dit)
    tkw = dict(lr=1e-2, latent_mean=0.05, latent_scale=0.8, ema_decay=0.9)       # an EMA that moves visibly within a step
    g = torch.Generator(device=DEV).manual_seed(0)
    images = torch.rand(4, 3, 256, 256, device=DEV, generator=g) * 2 - 1
    labels = torch.tensor([3, 7, 1, 9], device=DEV)
    ys = torch.tensor([2, 8], device=DEV)
    noise = torch.randn(2, 32, 16, 16, device=DEV, generator=g)

    def by_hand(tr, cfg_scale, decode):
        m2 = LightningDiT(**dkw).to(DEV)
        m2.load_state_dict(tr.ema_state_dict(), strict=True)
        m2 = m2.eval().requires_grad_(False)
        fn = Sampler(tr.transport).sample_ode(sampling_method="euler", num_steps=5)
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            if cfg_scale > 1.0:
                s = fn(torch.cat([noise, noise]), m2.forward_with_cfg, y=torch.cat([ys, torch.full_like(ys, 10)]), cfg_scale=cfg_scale, standard_cfg=True)[-1]
                s = s.chunk(2, dim=0)[0]
            else:
                s = fn(noise, m2.forward, y=ys)[-1]
            tok = dit_output_to_tokens(s, 0.05, 0.8)
            return vae.decode(tok).float() if decode else tok.float()

    def state(tr):
        tr.wait_optimizers()
        return [tr.fp.flat.clone(), tr.fp.ema.clone(), tr.opt.exp_avg.clone(), tr.opt.exp_avg_sq.clone()]

    # A: four steps.  B: two steps, samples (one of them drawing its own noise), two steps.
    tr_a = DiffusionTrainer(dit, vae, **tkw)
    for s in range(4):
        torch.manual_seed(100 + s)
        tr_a.step(images, labels)
    want = state(tr_a)
    tr = DiffusionTrainer(dit_b, vae, **tkw)
    for s in range(2):
        torch.manual_seed(100 + s)
        tr.step(images, labels)
    assert dit_b.training
    first = tr.sample(ys, noise, cfg_scale=2.5, sampling_method="euler", num_steps=5, decode=False)
    assert dit_b.training and first.shape == (2, 256, 32) and torch.isfinite(first).all()
    assert torch.equal(first, by_hand(tr, 2.5, False))
    img = tr.sample(ys, noise, cfg_scale=2.5, sampling_method="euler", num_steps=5)
    assert img.shape == (2, 3, 256, 256) and img.dtype == torch.float32 and torch.equal(img, by_hand(tr, 2.5, True))
    own = tr.sample(ys, cfg_scale=2.5, sampling_method="euler", num_steps=5, decode=False)                 # noise from the call's own generator
    assert own.shape == first.shape and not torch.equal(own, first)
    # cfg_scale 1: the unguided branch -- the by-hand run with n labels and the n-sample state, model.forward
    plain = tr.sample(ys, noise, cfg_scale=1.0, sampling_method="euler", num_steps=5, decode=False)
    assert torch.equal(plain, by_hand(tr, 1.0, False)) and not torch.equal(plain, first)
    dit_b.eval()
    tr.sample(ys, noise, cfg_scale=2.5, sampling_method="euler", num_steps=2, decode=False)
    assert not dit_b.training
    for s in range(2, 4):
        torch.manual_seed(100 + s)
        tr.step(images, labels)
    got = state(tr)
    for a, b, name in zip(got, want, ("weights", "ema", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a, b), name
    assert tr.opt.t == tr_a.opt.t and tr.train_steps == 4
    # the EMA has moved: the next sample follows it
    second = tr.sample(ys, noise, cfg_scale=2.5, sampling_method="euler", num_steps=5, decode=False)
    assert not torch.equal(second, first) and torch.equal(second, by_hand(tr, 2.5, False))
    # the reference's defaults (dopri5, cfg_scale 4): finishes, finite images
    img = tr.sample(ys)
    assert img.shape == (2, 3, 256, 256) and torch.isfinite(img).all()
