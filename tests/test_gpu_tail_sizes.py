"""The loss and optimiser tail kernels at sizes past their launchers' grid caps -- the grid-stride loops run several sweeps -- and at their ragged tails,
against float64 on the SAME f32 / bf16 operands and f32-rounded scalars (-m gpu).

  grad_norm        cap 2048 blocks x 256 x 4 = 2,097,152 elements per sweep; the n & 3 tail; accumulate_prev
  adamw_ema_step   cap 8192 x 256 x 4 = 8,388,608; the n & 3 tail; ema = None; norm_out = None; the bf16 shadow
  l1_mse           cap 2,097,152
  dmd_pre          cap 524,288 elements, the sample index changing inside a sweep
  dmd_post         batch > 64 (dmd_final_kernel's lane loop), per_sample no multiple of 256
  lpips_diff       C = 72 (nine live channel lanes of sixteen), ragged pixel chunks, batch 70; lpips_diff_pool against float64 as well

Worst figures observed on an MI355X (bar in brackets):
  grad_norm        norm 3.6e-08, clip coefficient 3.3e-08, two buffers 9.3e-09 relative [1e-6]
  adamw_ema_step   p 5.5e-08, m 5.0e-08, ema 9.0e-08 elem_err [1e-6]; v 2.2e-07 relative [1e-6]; shadow and shadow-less state bit-equal
  l1_mse           L1 2.9e-08, MSE 3.2e-08 relative [1e-6]; gradient 7.8e-08 relative per element [1e-6]
  dmd_pre          elem_err 1.3e-07, rel_err 5.9e-08 [1e-6]
  dmd_post         loss 5.5e-08, gradient norm 4.1e-08 relative [1e-4]; dlatents rel_err 6.8e-07 [1e-4]
  lpips_diff       value 7.5e-08 relative [1e-5]; gradient rel_err 3.3e-03 [4e-3]
  lpips_diff_pool  value 1.7e-08 relative [1e-5]; gradient rel_err 2.1e-03 [4e-3]; pooled features bit-equal
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import elem_err, rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _ops():
    from dmvae_amd import ops
    return ops


def _f32(v):
    return float(np.float32(v))


def _fig(what, e, bar):
    print(f"[fig] {what}: {e:.2e} (bar {bar:.0e})")
    return e


# ---- grad_norm ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5, 1023, 3 * 2097152 + 3])
def test_grad_norm_sizes(n):
    ops = _ops()
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen) * 0.3 + 0.01
    gd = g.to(DEV)
    ref = g.double().pow(2).sum().sqrt().item()
    for factor in (2.0, 0.37):                       # below max_norm: no clipping; above: clipped
        max_norm = _f32(factor * ref)
        out = ops.grad_norm(gd, max_norm)
        nrm, coef, sq = out.tolist()
        e = _fig(f"grad_norm n {n} norm", abs(nrm - ref) / ref, 1e-6)
        assert e <= 1e-6
        assert abs(sq - ref * ref) <= 2e-6 * ref * ref
        if factor > 1:
            assert coef == 1.0
        else:
            want = max_norm / (ref + _f32(1e-6))
            e = _fig(f"grad_norm n {n} clip coefficient", abs(coef - want) / want, 1e-6)
            assert coef < 1.0 and e <= 1e-6
        assert torch.equal(ops.grad_norm(gd, max_norm), out)       # fixed-order sums: a rerun gives the same bits


@pytest.mark.parametrize("na,nb", [(3, 5), (1023, 2 * 2097152 + 1), (2 * 2097152 + 1028, 7)])
def test_grad_norm_two_buffers(na, nb):
    ops = _ops()
    gen = torch.Generator().manual_seed(na + nb)
    a, b = torch.randn(na, generator=gen) * 0.2, torch.randn(nb, generator=gen) * 0.5
    ref = torch.cat([a, b]).double().pow(2).sum().sqrt().item()
    out = torch.full((3,), 123.0, device=DEV)              # stale contents: the first buffer overwrites them
    ops.grad_norm(a.to(DEV), 1.0, norm_out=out)
    ra = a.double().pow(2).sum().sqrt().item()
    assert abs(out[0].item() - ra) <= 1e-6 * ra
    res = ops.grad_norm(b.to(DEV), 1.0, norm_out=out, accumulate_prev=True)
    assert res is out
    e = _fig(f"grad_norm two buffers {na} + {nb}", abs(out[0].item() - ref) / ref, 1e-6)
    assert e <= 1e-6
    want = min(1.0, 1.0 / (out[0].item() + _f32(1e-6)))
    assert abs(out[1].item() - want) <= 1e-6 * want


# ---- adamw_ema_step ------------------------------------------------------------------------------------------------------------------------------------------
HYPER = dict(lr=3e-4, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.005, decay=0.9999)
BIG = 8388608 + 4 * 4099 + 3


@functools.lru_cache(maxsize=None)
def _adam_state(n):
    gen = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 0.1
    m = torch.randn(n, generator=gen) * 0.05
    v = torch.rand(n, generator=gen) * 0.01
    ema = p + torch.randn(n, generator=gen) * 0.01
    return p, g, m, v, ema


def _adam_ref(n, step, coef, with_ema):
    p, g, m, v, ema = (t.double() for t in _adam_state(n))
    h = {k: _f32(x) for k, x in HYPER.items()}
    p2, m2, v2 = R.adamw_step(p, g * coef, m, v, step, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"])
    return p2, m2, v2, (R.ema_update(ema, p2, h["decay"]) if with_ema else None)


def _adam_run(n, step, norm_out, with_ema, with_shadow):
    ops = _ops()
    p, g, m, v, ema = (t.to(DEV) for t in _adam_state(n))        # fresh device copies: the step works in place
    ema = ema if with_ema else None
    shadow = torch.full((n,), float("nan"), dtype=BF, device=DEV) if with_shadow else None
    ops.adamw_ema_step(p, g, m, v, ema, norm_out, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["wd"], step, HYPER["decay"], shadow=shadow)
    assert torch.equal(g.cpu(), _adam_state(n)[1])               # the gradient is read only
    return p, m, v, ema, shadow


def _adam_check(n, step, clip, with_ema):
    coef = 0.4321 if clip else 1.0
    norm_out = torch.tensor([1.0 / 0.4321, coef, 5.0], device=DEV) if clip else None
    coef = _f32(coef)
    p, m, v, ema, _ = _adam_run(n, step, norm_out, with_ema, False)
    ps, ms, vs, emas, shadow = _adam_run(n, step, norm_out, with_ema, True)
    # the shadow-writing entry: the same f32 state bit for bit, plus bf16(new weight)
    assert torch.equal(ps, p) and torch.equal(ms, m) and torch.equal(vs, v) and (ema is None or torch.equal(emas, ema))
    assert torch.equal(shadow.view(torch.int16), p.to(BF).view(torch.int16))
    rp, rm, rv, rema = _adam_ref(n, step, coef, with_ema)
    tag = f"adamw n {n} step {step} clip {clip} ema {with_ema}"
    e_p, e_m = _fig(tag + " p elem_err", elem_err(p.cpu(), rp), 1e-6), _fig(tag + " m elem_err", elem_err(m.cpu(), rm), 1e-6)
    e_v = _fig(tag + " v relative", ((v.cpu().double() - rv).abs() / rv).max().item(), 1e-6)
    assert e_p < 1e-6 and e_m < 1e-6 and e_v <= 1e-6
    if with_ema:
        assert _fig(tag + " ema elem_err", elem_err(ema.cpu(), rema), 1e-6) < 1e-6
    else:
        assert ema is None and emas is None


@pytest.mark.parametrize("n", [1, 2, 3, 7, 1027])
def test_adamw_ema_step_tails(n):
    for step in (1, 7):
        for clip in (True, False):
            for with_ema in (True, False):
                _adam_check(n, step, clip, with_ema)


@pytest.mark.parametrize("step,clip,with_ema", [(7, True, True), (1, False, False)])
def test_adamw_ema_step_past_the_cap(step, clip, with_ema):
    _adam_check(BIG, step, clip, with_ema)


# ---- l1_mse --------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _l1_inputs():
    n = 2 * 2097152 + 4 * 333
    gen = torch.Generator().manual_seed(17)
    images = torch.rand(n, generator=gen) * 2 - 1
    recon = images + 0.2 * torch.randn(n, generator=gen)
    same = torch.tensor([0, 5, 2097152, n // 2 + 1, n - 1333, n - 1])       # planted recon == images: the first element of the second sweep and the last one among them
    recon[same] = images[same]
    return recon, images, same


@pytest.mark.parametrize("w1,w2", [(1.0, 0.5), (1.0, 0.0), (0.0, 2.0)])
def test_l1_mse_past_the_cap(w1, w2):
    ops = _ops()
    recon, images, same = _l1_inputs()
    n = recon.numel()
    rd, im = recon.to(DEV), images.to(DEV)
    out, grad = ops.l1_mse(rd, im, w1, w2)
    d = recon.double() - images.double()
    l1, l2 = R.l1_mse(recon.double(), images.double())
    e1, e2 = _fig(f"l1_mse ({w1}, {w2}) L1", abs(out[0].item() - l1.item()) / l1.item(), 1e-6), _fig(f"l1_mse ({w1}, {w2}) MSE", abs(out[1].item() - l2.item()) / l2.item(), 1e-6)
    assert e1 <= 1e-6 and e2 <= 1e-6
    gref = _f32(w1) * torch.sign(d) / n + 2 * _f32(w2) * d / n
    gc = grad.cpu().double()
    live = d != 0
    e = _fig(f"l1_mse ({w1}, {w2}) gradient, relative per element", ((gc - gref).abs()[live] / gref.abs()[live]).max().item(), 1e-6)
    assert e <= 1e-6
    assert (~live).sum().item() >= same.numel() and (gc[~live] == 0).all() and (gc[same] == 0).all()
    out2, none = ops.l1_mse(rd, im, w1, w2, need_grad=False)
    assert none is None and torch.equal(out2, out)


# ---- DMD -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_dmd_pre_past_the_cap():
    ops = _ops()
    b, per = 5, 131075
    gen = torch.Generator().manual_seed(23)
    x1, x0 = torch.randn(b, per, generator=gen), torch.randn(b, per, generator=gen)
    t = torch.rand(b, generator=gen) * 0.9 + 0.05
    xt = ops.dmd_pre(x1.to(DEV), x0.to(DEV), t.to(DEV))
    ref, _ = R.transport_plan(t.double(), x0.double(), x1.double())
    assert _fig("dmd_pre elem_err", elem_err(xt.cpu(), ref), 1e-6) < 1e-6
    assert _fig("dmd_pre rel_err", rel_err(xt.cpu(), ref), 1e-6) < 1e-6


@functools.lru_cache(maxsize=None)
def _dmd_inputs():
    b, per = 130, 1000
    gen = torch.Generator().manual_seed(29)
    x1, x0 = torch.randn(b, per, generator=gen), torch.randn(b, per, generator=gen)
    t = torch.rand(b, generator=gen) * 0.9 + 0.05
    vs = [torch.randn(b, per, generator=gen) for _ in range(4)]
    xt = R.transport_plan(t.double(), x0.double(), x1.double())[0].float()
    return x1, x0, t, xt, vs


@pytest.mark.parametrize("weight_factor", [True, False])
@pytest.mark.parametrize("cfg", [1.0, 4.5])
def test_dmd_post_wide_batch(cfg, weight_factor):
    ops = _ops()
    x1, x0, t, xt, (vt, vst, vtu, vsu) = _dmd_inputs()
    loss, gnorm, grad = R.dmd_loss(x1.double(), t.double(), x0.double(), vt.double(), vst.double(), vtu.double(), vsu.double(), cfg=cfg, weight_factor=weight_factor)
    d = lambda a: a.to(DEV)
    out, dl = ops.dmd_post(d(x1), d(xt), d(t), d(vt), d(vst), d(vtu), d(vsu), cfg=cfg, weight_factor=weight_factor)
    tag = f"dmd_post cfg {cfg} weight_factor {weight_factor}"
    e_l = _fig(tag + " loss", abs(out[0].item() - loss.item()) / loss.item(), 1e-4)
    e_n = _fig(tag + " gradient norm", abs(out[1].item() - gnorm.item()) / gnorm.item(), 1e-4)
    e_d = _fig(tag + " dlatents rel_err", rel_err(dl.cpu(), grad / grad.numel()), 1e-4)
    assert e_l < 1e-4 and e_n < 1e-4 and e_d < 1e-4
    if cfg == 1.0:        # the unconditional outputs are not read then
        out2, dl2 = ops.dmd_post(d(x1), d(xt), d(t), d(vt), d(vst), cfg=cfg, weight_factor=weight_factor)
        assert torch.equal(out2, out) and torch.equal(dl2, dl)


# ---- LPIPS level ---------------------------------------------------------------------------------------------------------------------------------------------
LPIPS_CASES = [(3, 37, 41, 64), (2, 10, 10, 72), (70, 3, 11, 512), (1, 64, 64, 128)]


@functools.lru_cache(maxsize=None)
def _lpips_ref(n, h, w_, c):
    gen = torch.Generator().manual_seed(n + h + w_ + c)
    f0 = torch.relu(torch.randn(n, h, w_, c, generator=gen)).to(BF)
    f1 = torch.relu(torch.randn(n, h, w_, c, generator=gen)).to(BF)
    lin = torch.rand(c, generator=gen)
    a = f0.double().permute(0, 3, 1, 2)
    b = f1.double().permute(0, 3, 1, 2).requires_grad_(True)
    val = R.lpips_from_feats([a], [b], [lin.double()])
    (grad,) = torch.autograd.grad(val, b)
    return f0, f1, lin, val.item(), grad.permute(0, 2, 3, 1)


def _lpips_bars(tag, out, df, val, grad, preset=0.0):
    e_v = _fig(tag + " value", abs(out.item() - preset - val) / val, 1e-5)
    e_g = _fig(tag + " gradient rel_err", rel_err(df.float().cpu(), grad), 4e-3)
    assert e_v < 1e-5 and e_g < 4e-3


@pytest.mark.parametrize("case", LPIPS_CASES)
def test_lpips_diff_float64(case):
    ops = _ops()
    n, h, w_, c = case
    f0, f1, lin, val, grad = _lpips_ref(*case)
    a, b, lw = f0.to(DEV), f1.to(DEV), lin.to(DEV)
    gscale = 1.0 / (h * w_ * n)
    out = torch.full((1,), 7.0, device=DEV)                      # stale contents: accumulate=False overwrites them
    df = ops.lpips_diff(a, b, lw, out, gscale, True, accumulate=False)
    _lpips_bars(f"lpips_diff {case}", out, df, val, grad)
    out_acc = torch.full((1,), 0.25, device=DEV)
    df2 = ops.lpips_diff(a, b, lw, out_acc, gscale, True, accumulate=True)
    assert torch.equal(df2, df)
    _lpips_bars(f"lpips_diff {case} accumulating onto 0.25", out_acc, df2, val, grad, preset=0.25)
    out_ng = torch.zeros(1, device=DEV)
    assert ops.lpips_diff(a, b, lw, out_ng, gscale, False, accumulate=False) is None and torch.equal(out_ng, out)
    same = torch.full((1,), 7.0, device=DEV)
    dz = ops.lpips_diff(b, b.clone(), lw, same, gscale, True, accumulate=False)
    assert same.item() == 0.0 and (dz == 0).all()                # LPIPS(x, x) is exactly zero, and so is its gradient


@pytest.mark.parametrize("case", [c for c in LPIPS_CASES if c[1] % 2 == 0 and c[2] % 2 == 0])
def test_lpips_diff_pool_float64(case):
    ops = _ops()
    n, h, w_, c = case
    f0, f1, lin, val, grad = _lpips_ref(*case)
    hcat = torch.cat([f0, f1]).to(DEV)
    out = torch.full((1,), 0.25, device=DEV)
    df, pooled = ops.lpips_diff_pool(hcat, n, lin.to(DEV), out, 1.0 / (h * w_ * n), True, accumulate=True)
    _lpips_bars(f"lpips_diff_pool {case} accumulating onto 0.25", out, df, val, grad, preset=0.25)
    want = F.max_pool2d(torch.cat([f0, f1]).float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(pooled.float().cpu(), want)
