"""GPU: the multi-tensor optimiser tail (csrc/optim_mt.hip, ops.mt_*, optim.AdamW / clip_grad_norm_ / update_ema) -- the reference's own loop
(train_tokenizer.py:140-150,382,415-419,437) over ordinary, separately allocated parameters.  The kernels are held to the flat kernels of csrc/optim.hip bit for
bit (one per-element function compiled into both), the norm to float64, the public objects to the reference's own optimiser run (tests/golden/opt_tail.npz), to
torch.optim.AdamW through a state_dict() hand-over, to the caches of functional.py, and to the reference's four-step capture in the loop shape its scripts have."""
import copy
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sizes():
    from dmvae_amd import ops
    c = ops.mt_chunk_elems()
    return [0, 1, 3, 4, 5, 1023, c - 1, c, c + 1, 2 * c + 7]


def _alloc(n, offset, gen, scale=1.0):
    """A 1-D f32 tensor of n elements in its own buffer; offset 1: a view that starts one element in (4-byte aligned only)."""
    t = (torch.randn(n + offset, generator=gen) * scale).to(DEV)[offset:]
    assert t.numel() == n and (n == 0 or t.data_ptr() % 16 == 4 * offset)
    return t


LISTS = ["aligned", "views", "single"]


def _tensor_list(kind, gen, scale=1.0):
    if kind == "single":
        return [_alloc(_sizes()[-1], 0, gen, scale)]
    return [_alloc(n, 1 if kind == "views" else 0, gen, scale) for n in _sizes()]


def _flat(ts):
    """The 16-byte-padded concatenation (optim.FlatParams' layout) and each tensor's offset in it."""
    offs, n = [], 0
    for t in ts:
        offs.append(n)
        n += (t.numel() + 3) // 4 * 4
    flat = torch.zeros(max(n, 4), dtype=torch.float32, device=DEV)
    for t, o in zip(ts, offs):
        flat[o:o + t.numel()] = t
    return flat, offs


def _bits_equal(ts, flat, offs):
    return all(torch.equal(t.view(torch.int32), flat[o:o + t.numel()].view(torch.int32)) for t, o in zip(ts, offs))


@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("scale", [1.0, 1e3])
def test_mt_grad_norm_vs_float64(kind, scale):
    """||g|| over the list against float64 of the same gradients: relative error <= 1e-6.  An emulation of the kernel's summation order on the CPU (f32 per lane,
    wave butterfly, four waves per chunk, f64 over the chunk partials, f32 result) gave 5.3e-8 at worst over these lists, randn and randn x 1e3, six seeds: the
    bar has room to spare.  Two calls give equal bits; the clip coefficient is min(1, max_norm / (norm + 1e-6)) formed in f32 from the norm."""
    from dmvae_amd import ops
    gen = torch.Generator().manual_seed(11)
    gs = _tensor_list(kind, gen, scale)
    want = float(np.sqrt(sum(float((g.double() ** 2).sum().item()) for g in gs)))
    for max_norm in (1.0, 1e9):
        out = ops.mt_grad_norm(gs, max_norm)
        again = ops.mt_grad_norm(gs, max_norm)
        assert torch.equal(out.view(torch.int32), again.view(torch.int32))
        norm = out[0].item()
        print(f"mt_grad_norm {kind} x{scale:g}: {norm!r} vs f64 {want!r}: rel {abs(norm - want) / want:.3e}")
        assert abs(norm - want) <= 1e-6 * want
        coef = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
        assert out[1].item() == float(min(np.float32(1.0), coef))
        assert abs(out[2].item() - want * want) <= 2e-6 * want * want
    assert ops.mt_grad_norm([torch.zeros(0, device=DEV), torch.zeros(0, device=DEV)], 1.0).tolist() == [0.0, 1.0, 0.0]     # only empty tensors


@pytest.mark.parametrize("kind", LISTS)
def test_mt_scale_grads_is_one_f32_multiply(kind):
    from dmvae_amd import ops
    gen = torch.Generator().manual_seed(12)
    gs = _tensor_list(kind, gen, 30.0)
    norm3 = ops.mt_grad_norm(gs, 1.0)
    assert 0 < norm3[1].item() < 1
    want = [g * norm3[1] for g in gs]
    ops.mt_scale_grads(gs, norm3)
    assert all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(gs, want))


@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("wd", [0.0, 0.005])
@pytest.mark.parametrize("with_ema", [False, True])
def test_mt_adamw_ema_step_equals_the_flat_kernel_bit_for_bit(kind, wd, with_ema):
    """Steps 1 to 3 on the separate tensors against ops.adamw_ema_step on their 16-byte-padded concatenation, both fed the same norm_out3."""
    from dmvae_amd import ops
    gen = torch.Generator().manual_seed(13)
    ps = _tensor_list(kind, gen)
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    off = 1 if kind == "views" else 0
    es = [_alloc(p.numel(), off, gen) for p in ps] if with_ema else None
    fp, offs = _flat(ps)
    fm, fv = torch.zeros_like(fp), torch.zeros_like(fp)
    fe = _flat(es)[0] if with_ema else None
    for step in (1, 2, 3):
        gs = _tensor_list(kind, gen, 3.0)
        fg, _ = _flat(gs)
        norm3 = ops.mt_grad_norm(gs, 1.0)
        ops.mt_adamw_ema_step(ps, gs, ms, vs, es, norm3, 1e-3 * step, 0.9, 0.95, 1e-8, wd, step, 0.9999)
        ops.adamw_ema_step(fp, fg, fm, fv, fe, norm3, 1e-3 * step, 0.9, 0.95, 1e-8, wd, step, 0.9999)
        assert _bits_equal(ps, fp, offs), ("p", step)
        assert _bits_equal(ms, fm, offs), ("m", step)
        assert _bits_equal(vs, fv, offs), ("v", step)
        if with_ema:
            assert _bits_equal(es, fe, offs), ("ema", step)
    assert all(torch.isfinite(p).all() for p in ps)
    if with_ema:        # a record without an EMA in a table that has them: that tensor's EMA stays out, the others move
        es2 = [None if i % 2 else e for i, e in enumerate(es)]
        kept = [e.clone() for e in es]
        gs = _tensor_list(kind, gen, 3.0)
        ops.mt_adamw_ema_step(ps, gs, ms, vs, es2, None, 1e-3, 0.9, 0.95, 1e-8, wd, 4, 0.5)
        for i, (e, k) in enumerate(zip(es, kept)):
            assert torch.equal(e, k) == (i % 2 == 1 or e.numel() == 0)


@pytest.mark.parametrize("kind", LISTS)
def test_mt_ema_equals_the_flat_kernels_ema_line(kind):
    """The flat kernel at lr 0, zero gradient and zero state leaves p as it is and runs its EMA line alone; decay 0 returns p exactly."""
    from dmvae_amd import ops
    gen = torch.Generator().manual_seed(14)
    ps = _tensor_list(kind, gen)
    off = 1 if kind == "views" else 0
    es = [_alloc(p.numel(), off, gen) for p in ps]
    fp, offs = _flat(ps)
    fe = _flat(es)[0]
    zero = lambda: torch.zeros_like(fp)
    for decay in (0.9999, 0.5):
        ops.mt_ema(es, ps, decay)
        ops.adamw_ema_step(fp, zero(), zero(), zero(), fe, None, 0.0, 0.9, 0.95, 1e-8, 0.0, 1, decay)
        assert _bits_equal(ps, fp, offs) and _bits_equal(es, fe, offs), decay
    ops.mt_ema(es, ps, 0.0)
    assert all(torch.equal(e.view(torch.int32), p.view(torch.int32)) for e, p in zip(es, ps))


def _opt_tail_model(g):
    names = ["0.weight", "0.bias", "2.weight", "2.bias"]
    shapes = [g["p0." + n].shape for n in names]
    net = torch.nn.Sequential(torch.nn.Linear(shapes[0][1], shapes[0][0]), torch.nn.SiLU(), torch.nn.Linear(shapes[2][1], shapes[2][0]))
    net.load_state_dict({n: g.t("p0." + n) for n in names})
    return names, net.to(DEV)


def test_public_objects_reproduce_the_references_optimiser_run():
    """optim.AdamW + optim.clip_grad_norm_ + optim.update_ema + LambdaLR over six steps of tests/golden/opt_tail.npz (the reference's clip_grad_norm_, AdamW,
    LambdaLR and update_ema on the same gradients): norms within 1e-5, final weights and EMA within rel 1e-6 -- the bars the flat kernel is held to -- lrs exact."""
    from dmvae_amd import optim
    g = load_golden("opt_tail")
    names, net = _opt_tail_model(g)
    ema_net = copy.deepcopy(net).requires_grad_(False)
    warm = int(g["warmup_steps"])
    opt = optim.AdamW(net.parameters(), lr=1e-4, weight_decay=0.005, betas=(0.9, 0.95), eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: s / warm if s < warm else 1.0)
    params = dict(net.named_parameters())
    for it in range(6):
        for i, n in enumerate(names):
            params[n].grad = g.t(f"g{it}.{i}").to(DEV)
        norm = optim.clip_grad_norm_(net.parameters(), max_norm=1.0)
        assert norm.dim() == 0 and norm.is_cuda
        assert abs(norm.item() - float(g["norms"][it])) < 1e-5 * float(g["norms"][it])
        assert opt.param_groups[0]["lr"] == float(g["lrs"][it])
        opt.step()
        opt.zero_grad(set_to_none=True)
        sched.step()
        optim.update_ema(ema_net, net)
    ema = dict(ema_net.named_parameters())
    for n in names:
        assert rel_err(params[n].detach().cpu(), g.t("p6." + n)) < 1e-6, n
        assert rel_err(ema[n].detach().cpu(), g.t("ema6." + n)) < 1e-6, n
    st = opt.state[params[names[0]]]
    assert list(st) == ["step", "exp_avg", "exp_avg_sq"] and not st["step"].is_cuda and float(st["step"]) == 6.0


def test_state_dict_interchanges_with_torch_adamw():
    """Two steps with ours, state_dict() into a fresh torch.optim.AdamW on cloned parameters, one more step on each side: the loaded state is bit-equal, the
    results agree within rel 1e-6.  And back: torch's state into a fresh one of ours."""
    from dmvae_amd import optim
    g = load_golden("opt_tail")
    names, net = _opt_tail_model(g)
    kw = dict(lr=1e-3, weight_decay=0.005, betas=(0.9, 0.95), eps=1e-8)
    ours = optim.AdamW(net.parameters(), **kw)
    params = dict(net.named_parameters())

    def feed(prm, it):
        for i, n in enumerate(names):
            prm[n].grad = g.t(f"g{it}.{i}").to(DEV)

    for it in range(2):
        feed(params, it)
        ours.step()
    twin = copy.deepcopy(net)
    tparams = dict(twin.named_parameters())
    stock = torch.optim.AdamW(twin.parameters(), **kw)
    sd = ours.state_dict()
    stock.load_state_dict(copy.deepcopy(sd))
    for i, n in enumerate(names):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            a, b = stock.state[tparams[n]][k], sd["state"][i][k]
            assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), (n, k)
    back = copy.deepcopy(net)
    bparams = dict(back.named_parameters())
    ours2 = optim.AdamW(back.parameters(), **kw)
    ours2.load_state_dict(copy.deepcopy(stock.state_dict()))
    for prm, o in ((params, ours), (tparams, stock), (bparams, ours2)):
        feed(prm, 2)
        o.step()
    for n in names:
        assert rel_err(params[n].detach(), tparams[n].detach()) < 1e-6, n
        assert torch.equal(params[n].detach(), bparams[n].detach()), n
        assert float(stock.state[tparams[n]]["step"]) == float(ours.state[params[n]]["step"]) == float(ours2.state[bparams[n]]["step"]) == 3.0


def _small_decoder(seed):
    from dmvae_amd.models.flux_ae import Decoder
    torch.manual_seed(seed)
    dec = Decoder(ch=32, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, in_channels=3, resolution=256, z_channels=16)
    dec.post_init(z_channels=32)
    return dec


def _fresh_like(dec):
    new = _small_decoder(99)
    new.load_state_dict(dec.state_dict())
    return new.to(DEV)


def test_caches_of_packed_operands_follow_the_raw_pointer_updates():
    """functional.packed / _bf key on (data_ptr, _version); the kernels write weights through raw pointers, so step() and update_ema() bump the version by hand.
    forward, backward, step(), forward again: the second output is bit-equal to a fresh module's that was loaded with the updated weights -- and not to the first
    output, which is what a stale cache returns.  The same for an EMA model after update_ema."""
    from dmvae_amd import optim
    dec = _small_decoder(5).to(DEV)
    ema = _fresh_like(dec).requires_grad_(False)
    z = torch.randn(2, 32, 4, 4, generator=torch.Generator().manual_seed(6)).to(DEV)
    opt = optim.AdamW(dec.parameters(), lr=1e-2, weight_decay=0.005, betas=(0.9, 0.95))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out0 = dec(z).float()
        out0.abs().mean().backward()
        with torch.no_grad():
            ema0 = ema(z).float()
        optim.clip_grad_norm_(dec.parameters(), 1.0)
        versions = [p._version for p in dec.parameters()]
        opt.step()
        assert all(p._version > v for p, v in zip(dec.parameters(), versions))
        with torch.no_grad():
            out1 = dec(z).float()
            want1 = _fresh_like(dec)(z).float()
        assert not torch.equal(out1, out0.detach())
        assert torch.equal(out1, want1)
        optim.update_ema(ema, dec, decay=0.5)
        with torch.no_grad():
            ema1 = ema(z).float()
            want_ema = _fresh_like(ema).requires_grad_(False)(z).float()
        assert not torch.equal(ema1, ema0) and not torch.equal(ema1, out1)
        assert torch.equal(ema1, want_ema)


def _reference_loop(tail, g):
    """Four steps in the shape of train_tokenizer.py:403-437 -- autocast around forward, backward and the optimiser step; clip + .item();
    zero_grad(set_to_none=True); LambdaLR; update_ema on a deepcopy -- over dmvae_amd's VAE + LPIPS + losses; no TokenizerTrainer, no flat buffers.
    tail: "hip" = optim.AdamW / clip_grad_norm_ / update_ema, "stock" = torch's own and the scripts' Python EMA loop."""
    from dmvae_amd import losses, optim
    from dmvae_amd.utils.lpips import LPIPS
    from test_oracle_golden import lpips_params
    from test_oracle_step import step_small_inputs
    p, vae, names, images = step_small_inputs(g)
    vae.load_state_dict(p, strict=True)
    vae = vae.to(DEV)
    vae.encoder.eval()
    vae.encoder.requires_grad_(False)                              # train_tokenizer.py:295-297
    lp = LPIPS().eval().requires_grad_(False)
    missing = lp.load_state_dict(lpips_params(g, "lp."), strict=False)
    assert not missing.unexpected_keys and all("scaling_layer" in k for k in missing.missing_keys), missing
    lp = lp.to(DEV)
    hip = tail == "hip"
    adamw = optim.AdamW if hip else torch.optim.AdamW
    clip = optim.clip_grad_norm_ if hip else torch.nn.utils.clip_grad_norm_
    train = [q for q in vae.parameters() if q.requires_grad]
    opt = adamw(train, lr=float(g["base_lr"]), weight_decay=0.005, betas=(0.9, 0.95), eps=1e-8)
    warm = int(g["warmup_steps"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: s / warm if s < warm else 1.0)
    ema_model = copy.deepcopy(vae).requires_grad_(False).eval()
    x = images.to(DEV)
    logs = []
    for s in range(len(g["lr"])):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            recon = vae(x, return_latent=False)
            l1, l2 = losses.l1_mse(recon, x, 1.0, 0.0)
            lpv = lp(x, recon).mean()
            rec_loss = l1 * 1.0 + l2 * 0.0 + lpv * 1.0
            log = {"L1": l1.item(), "L2": l2.item(), "LPIPS": lpv.item(), "rec_loss": rec_loss.item(), "lr": opt.param_groups[0]["lr"]}
            rec_loss.backward()
            log["vae_norm"] = clip(vae.parameters(), max_norm=1.0).item()
            opt.step()
            opt.zero_grad(set_to_none=True)
            sched.step()
        if hip:
            optim.update_ema(ema_model, vae)
        else:
            with torch.no_grad():
                ema_params = dict(ema_model.named_parameters())
                for name, param in vae.named_parameters():
                    ema_params[name].mul_(0.9999).add_(param.data, alpha=1 - 0.9999)
        logs.append(log)
    p0 = {k: p[k].clone() for k in names}
    p1 = {k: q.detach().cpu() for k, q in vae.named_parameters() if k in p0}
    ema = {k: q.detach().cpu() for k, q in ema_model.named_parameters() if k in p0}
    return logs, p0, p1, ema, names


@pytest.fixture(scope="module")
def step_small():
    return load_golden("step_small_w256")


@pytest.mark.parametrize("tail", ["hip", "stock"])
def test_reference_loop_shape_vs_reference_capture(tail, step_small):
    """The drop-in route as an unedited script would drive it, against the reference's four-step capture (tests/golden/step_small_w256.npz) at exactly the bars
    tests/test_gpu_train_step.py::test_step_small_vs_reference_capture holds TokenizerTrainer to.  "stock" is the twin with torch's own tail on the same forward
    and backward kernels: the yardstick for what the bars measure (bf16 forward / backward), held to the same bars."""
    from test_oracle_step import check_step_small
    g = step_small
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logs, p0, p1, ema, names = _reference_loop(tail, g)
    for s, log in enumerate(logs):
        print(f"{tail} step {s}: rec_loss {log['rec_loss']:.6f} (capture {float(g['rec_loss'][s]):.6f})  vae_norm {log['vae_norm']:.5f} "
              f"(capture {float(g['vae_norm'][s]):.5f})  lr {log['lr']:.3e}")
    assert logs[0]["rec_loss"] == logs[1]["rec_loss"]            # the first optimiser step runs at lr 0
    assert logs[3]["rec_loss"] < logs[2]["rec_loss"] < logs[1]["rec_loss"]
    assert sorted(ema) == sorted(names)
    check_step_small(g, logs, p0, p1, ema, names, len(logs) - 1, tol_loss=2e-2, tol_norm=5e-2, tol_abs_delta=5e-2, tol_signed=0.25, min_cos=0.9, tol_ema=0.5)


def test_patched_torch_objects_take_the_scripts_constructor_call():
    """After install_shadow(None, optim=True), in a child process: train_diffusion.py:209's call -- torch.optim.AdamW(..., weight_decay=0, fused=True) -- builds
    this build's optimiser; one step moves the parameters and leaves the parent's state keys (fused=True: `step` on the device, as the parent would hold it)."""
    code = r"""
import sys
sys.path.insert(0, %r)
import torch
import run_on_mi355x as L
L.install_shadow(None, optim=True)
import dmvae_amd.optim as ours
lin = torch.nn.Linear(48, 24).cuda()
before = [p.detach().clone() for p in lin.parameters()]
opt = torch.optim.AdamW(lin.parameters(), lr=1e-3, betas=(0.9, 0.95), weight_decay=0, fused=True)
assert type(opt) is ours.AdamW
lin(torch.randn(8, 48, device="cuda")).square().mean().backward()
norm = torch.nn.utils.clip_grad_norm_(lin.parameters(), 1.0)
assert norm.is_cuda and norm.item() > 0
for _ in range(2):
    opt.step()
assert all(not torch.equal(p.detach(), b) for p, b in zip(lin.parameters(), before))
for p in lin.parameters():
    st = opt.state[p]
    assert list(st) == ["step", "exp_avg", "exp_avg_sq"] and st["step"].is_cuda and st["step"].dtype == torch.float32 and st["step"].item() == 2.0
print("patched ok")
""" % ROOT
    env = {k: v for k, v in os.environ.items() if k != "DMVAE_ALLOW_STOCK"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "patched ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
