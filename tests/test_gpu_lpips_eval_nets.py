"""GPU: the evaluation LPIPS' net_type 'vgg' and 'squeeze' (evaluation/metrics.py:26-29) -- the two stride-2 maximum pools of dmvae_maxpool2d_f32 against
F.max_pool2d bit for bit, dmvae_lpips_head_form against dmvae_lpips_head (form 0, bit for bit) and numpy f64 (form 1, derived bound), and
dmvae_amd.models.lpips_eval.LPIPSVGG / LPIPSSqueeze against the f64 specification of tests/lpips_eval_nets_spec.py with seeded random parameters (neither
library nor a weight file is on any machine this package is developed on), their invariances, the training loss's exact twin, and the public interface.

Bounds.
  Pools: a maximum is exact; equality.
  Head, form 1 (u = 2^-53).  tests/test_gpu_lpips_eval.py derives B for form 0 from |n^ - n| <= k |n|, k = gamma_{c+5}: the sum s = sum_c f_c^2 carries
gamma_c, and eps + s, the root, the reciprocal and the product f r one rounding each.  Form 1 changes one operation: eps is added after the root instead
of before it, n = f * (1 / (sqrt(s) + eps)).  The root halves s's relative error and adds one rounding (<= gamma_{c+1}); sqrt(s) and eps are both
non-negative, so their sum keeps the larger operand's relative error and adds one rounding (<= gamma_{c+2}); the reciprocal and the product add one each:
gamma_{c+4} <= k.  Everything after n is unchanged, so the same B holds, and so does |kernel - numpy| <= 2.02 B (numpy's n is a single division).
  Whole networks: the criterion of tests/test_gpu_lpips_eval.py -- per tap and image the rel-L2 error of the f32 features against the f64 specification is
held to 8 e_ref, e_ref being the stock f32 CPU composition's error against the same f64 values, computed in the same run; the per-image value's relative
error to 8 x the largest feature e_ref of the run.
  Twin: the bf16 training loss against LPIPSVGG.from_training(m, normalize="reference")(a, b).mean() within 5e-3 relative, tests/test_gpu_lpips.py's own
tolerance for the value against its oracle.

Measured on an MI355X: profiles/lpips_eval_nets_accuracy.txt, DESIGN.md 3.9."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_eval_nets_spec as N
from test_gpu_lpips_eval import HEAD_SHAPES, SENTINEL, U64, gamma, head_inputs, nchw, nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NETS = ("vgg", "squeeze")
SIZES = {"vgg": [(16, 16), (35, 37), (64, 48)], "squeeze": [(25, 25), (35, 37), (64, 48)]}


# ---- 1. the pools ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(2, 2), (3, 3), (4, 5), (7, 8), (9, 11), (16, 13)])
@pytest.mark.parametrize("c", [4, 16, 48])
def test_pools_are_f_max_pool2d_bit_for_bit(h, w, c):
    """Batch 2, all-negative inputs (a maximum that started from 0 would show), written into channels [8, 8 + c) of a wider sentinel-filled buffer with
    rows to spare: the sentinel is untouched outside the slice.  (16, 13) x 48 is 1152 outputs: more than one block of 256."""
    from dmvae_amd import ops
    g = torch.Generator().manual_seed(100 * h + 10 * w + c)
    x = -(torch.rand(2, c, h, w, generator=g) * 9 + 0.5)
    x[0, :, 0, 0] = x[0, :, h - 1, w - 1]                             # a tie across one window (h, w <= 3)
    xd = nhwc(x).to(DEV)
    for kernel, ceil in ((2, False), (3, True)):
        if h < kernel or w < kernel:
            with pytest.raises(ValueError, match="maxpool2d_f32"):
                ops.maxpool2d_f32(xd, kernel, 2, ceil)
            continue
        want = nhwc(F.max_pool2d(x, kernel, 2, ceil_mode=ceil))
        ho, wo = want.shape[1:3]
        assert (ho, wo) == ((h // 2, w // 2) if kernel == 2 else (-(-(h - 3) // 2) + 1, -(-(w - 3) // 2) + 1))
        m, pitch = 2 * ho * wo, c + 20
        buf = torch.full((m + 3, pitch), SENTINEL, dtype=torch.float32, device=DEV)
        out = buf[:m].view(2, ho, wo, pitch)
        assert ops.maxpool2d_f32(xd, kernel, 2, ceil, out=out, c_offset=8).data_ptr() == out.data_ptr()
        host = buf.cpu()
        assert torch.equal(host[:m, 8:8 + c].reshape(2, ho, wo, c), want) and (want < 0).all()
        s = torch.tensor(SENTINEL)
        assert torch.equal(host[:m, :8], s.expand(m, 8)) and torch.equal(host[:m, 8 + c:], s.expand(m, 12)) and torch.equal(host[m:], s.expand(3, pitch))
        assert torch.equal(ops.maxpool2d_f32(xd, kernel, 2, ceil).cpu(), want)                # and a buffer of its own
    for kernel, stride, ceil in ((2, 2, True), (3, 2, False), (3, 1, True), (2, 1, False)):
        with pytest.raises(ValueError, match="not built"):
            ops.maxpool2d_f32(xd, kernel, stride, ceil)


# ---- 2. the head's two forms ------------------------------------------------------------------------------------------------------------------
def head_form(f, lin, eps, form, out=None, accumulate=False):
    """dmvae_lpips_head_form called directly (ops.lpips_head routes only form 1 to it)."""
    from dmvae_amd import _lib
    lib = _lib.lib()
    pairs, h, w, c = f.shape[0] // 2, *f.shape[1:]
    ws = torch.empty(max(lib.dmvae_lpips_head_workspace(pairs, h, w, c) // 8, 1), dtype=torch.float64, device=f.device)
    out = torch.empty(pairs, dtype=torch.float64, device=f.device) if out is None else out
    rc = lib.dmvae_lpips_head_form(f.data_ptr(), lin.data_ptr(), pairs, h, w, c, ctypes.c_double(eps), form, int(accumulate), ws.data_ptr(), out.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.dmvae_last_error()
    return out


def head_reference_form1(f, lin, eps):
    """numpy f64 -> (values [pairs], the bound B [pairs]): tests/test_gpu_lpips_eval.py's head_reference with the one changed operation."""
    x = f.numpy().astype(np.float64)
    pairs, (h, w, c) = x.shape[0] // 2, x.shape[1:]
    wl = lin.numpy().astype(np.float64)
    n1 = x[:pairs] / (np.sqrt((x[:pairs] * x[:pairs]).sum(-1, keepdims=True)) + eps)
    n2 = x[pairs:] / (np.sqrt((x[pairs:] * x[pairs:]).sum(-1, keepdims=True)) + eps)
    d = n1 - n2
    v = ((d * d) * wl).sum(-1).mean(axis=(1, 2))
    k = gamma(c + 5, U64)
    e = (k * (np.abs(n1) + np.abs(n2)) + U64 * np.abs(d)) * (1 + U64)
    t = np.abs(wl) * (2 * np.abs(d) * e + e * e + 2 * U64 * d * d)
    bound = (t.sum(axis=(1, 2, 3)) + gamma(c + h * w + 32, U64) * (np.abs(wl) * d * d).sum(axis=(1, 2, 3))) / (h * w) + 2 * U64 * np.abs(v)
    return torch.from_numpy(v), torch.from_numpy(1.01 * bound)


@pytest.mark.parametrize("pairs,h,w,c", HEAD_SHAPES)
def test_head_form0_is_lpips_head_bit_for_bit(pairs, h, w, c):
    from dmvae_amd import ops
    for signed in (False, True):
        f, lin = head_inputs(pairs, h, w, c, 13 * c + h + signed, signed)
        fd, ld = f.to(DEV), lin.to(DEV)
        for eps in (1e-8, 1e-6):
            assert torch.equal(head_form(fd, ld, eps, 0), ops.lpips_head(fd, ld, eps))
        start = torch.arange(pairs, dtype=torch.float64, device=DEV) * 0.37 + 1.25
        a, b = start.clone(), start.clone()
        head_form(fd, ld, 1e-8, 0, out=a, accumulate=True)
        ops.lpips_head(fd, ld, 1e-8, out=b, accumulate=True)
        assert torch.equal(a, b) and not torch.equal(a, start)
        assert torch.equal(ops.lpips_head(fd, ld, 1e-8, form=0), ops.lpips_head(fd, ld, 1e-8))


@pytest.mark.parametrize("pairs,h,w,c", HEAD_SHAPES)
@pytest.mark.parametrize("signed", [False, True])
def test_head_form1_against_f64_numpy(pairs, h, w, c, signed):
    from dmvae_amd import ops
    f, lin = head_inputs(pairs, h, w, c, 17 * c + h + signed, signed)
    if h * w > 1:
        f[:, 0, 0, :] = 0                                              # a pixel whose channels are all zero on both sides: adds 0, not NaN
    fd, ld = f.to(DEV), lin.to(DEV)
    want, bound = head_reference_form1(f, lin, 1e-10)
    got = ops.lpips_head(fd, ld, 1e-10, form=1)
    assert got.dtype == torch.float64 and tuple(got.shape) == (pairs,) and torch.isfinite(got).all()
    ratio = ((got.cpu() - want).abs() / (2 * bound)).max().item()
    print(f"lpips head form 1 {pairs} x {h} x {w} x {c} signed {signed}: value {want[0].item():+.6e}, max |err| / (2 B) {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(head_form(fd, ld, 1e-10, 1), got)                                   # ops routes form 1 to the entry
    big = ops.lpips_head(fd, ld, 1e-2, form=1).cpu()                                       # eps is an argument, and the form is not form 0
    want2, bound2 = head_reference_form1(f, lin, 1e-2)
    assert ((big - want2).abs() <= 2 * bound2).all() and not torch.equal(big, got.cpu())
    assert not torch.equal(ops.lpips_head(fd, ld, 1e-2), big.to(DEV))
    # identical halves: exactly 0.0; swapped halves: the same bits; all-zero images: 0.0; a rerun: the same bits
    zeros = torch.zeros(pairs, dtype=torch.float64, device=DEV)
    assert torch.equal(ops.lpips_head(torch.cat([fd[:pairs], fd[:pairs]]), ld, 1e-10, form=1), zeros)
    assert torch.equal(ops.lpips_head(torch.cat([fd[pairs:], fd[:pairs]]), ld, 1e-10, form=1), got)
    assert torch.equal(ops.lpips_head(torch.zeros_like(fd), ld, 1e-10, form=1), zeros)
    assert torch.equal(ops.lpips_head(fd, ld, 1e-10, form=1), got)
    i = pairs - 1
    assert torch.equal(ops.lpips_head(torch.cat([fd[i:i + 1], fd[pairs + i:pairs + i + 1]]), ld, 1e-10, form=1)[0], got[i])      # alone


# ---- 3. - 5. the whole networks -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sds():
    return {net: N.random_state_dict(net, 0) for net in NETS}


@pytest.fixture(scope="module")
def nets(sds):
    from dmvae_amd.models.lpips_eval import LPIPSSqueeze, LPIPSVGG
    out = {}
    for net, cls in (("vgg", LPIPSVGG), ("squeeze", LPIPSSqueeze)):
        out[net] = cls(chunk=2)
        out[net].load_state_dict(sds[net])
        out[net] = out[net].to(DEV)
    return out


@pytest.fixture(scope="module")
def spec(sds):
    """(net, h, w) -> (a, b, f64 values [3], f64 taps of both images, e_ref per tap [2 x 3] each); computed once, never modified."""
    out = {}
    for net in NETS:
        for h, w in SIZES[net]:
            a, b = N.image_pairs(3, h, w)
            v, t1, t2 = N.forward(net, sds[net], a, b)
            _, s1, s2 = N.forward(net, sds[net], a, b, torch.float32)
            taps = [torch.cat([x, y]) for x, y in zip(t1, t2)]
            eref = [N.rel_l2(torch.cat([x, y]), t) for x, y, t in zip(s1, s2, taps)]
            assert N.check_alive(v, t1, t2)[0] >= 0.25 and (v > 0).all() and torch.isfinite(v).all()
            out[(net, h, w)] = (a, b, v, taps, eref)
    return out


@pytest.mark.parametrize("net,h,w", [(net, h, w) for net in NETS for h, w in SIZES[net]])
def test_whole_network_against_the_f64_specification(nets, spec, net, h, w):
    """N = 3 with chunk = 2: a ragged last chunk.  Per tap and image e_hip <= 8 e_ref; per image the value's relative error <= 8 max e_ref.  Measured on
    an MI355X: profiles/lpips_eval_nets_accuracy.txt."""
    a, b, v64, taps64, eref = spec[(net, h, w)]
    m = nets[net]
    assert m.chunk == 2
    taps = m.taps(a.to(DEV), b.to(DEV))
    assert len(taps) == len(N.CHANNELS[net])
    worst_ref = max(e.max().item() for e in eref)
    for level, (f, f64, e_ref) in enumerate(zip(taps, taps64, eref)):
        assert tuple(f.shape) == (6, f64.shape[2], f64.shape[3], f64.shape[1])
        e_hip = N.rel_l2(nchw(f), f64)
        for i in range(6):
            print(f"lpips {net} accuracy {h} x {w} tap {level} image {'ab'[i // 3]}{i % 3}: e_hip {e_hip[i]:.3e} e_ref {e_ref[i]:.3e} ratio {e_hip[i] / e_ref[i]:.2f}")
        assert (e_hip <= 8 * e_ref).all(), level
    v = m(a.to(DEV), b.to(DEV)).cpu()
    assert v.dtype == torch.float64 and tuple(v.shape) == (3,)
    rel = (v - v64).abs() / v64
    for i in range(3):
        print(f"lpips {net} accuracy {h} x {w} value {i}: {v[i].item():.9e} (f64 {v64[i].item():.9e}) relative error {rel[i]:.3e} = {rel[i] / worst_ref:.2f} x "
              f"the largest feature e_ref {worst_ref:.3e}")
    assert (rel <= 8 * worst_ref).all()


def test_vgg_reference_normalisation_against_the_f64_specification(sds, spec):
    """normalize="reference": the same trunk (the taps are those of the test above), head form 1 with eps 1e-10; the value against the f64 specification's
    form 1 under the same criterion."""
    from dmvae_amd.models.lpips_eval import LPIPSVGG
    m = LPIPSVGG(chunk=2, normalize="reference")
    m.load_state_dict(sds["vgg"])
    m = m.to(DEV)
    for h, w in SIZES["vgg"]:
        a, b, v0, _, eref = spec[("vgg", h, w)]
        v64 = N.forward("vgg", sds["vgg"], a, b, form=1)[0]
        v = m(a.to(DEV), b.to(DEV)).cpu()
        worst_ref = max(e.max().item() for e in eref)
        rel = (v - v64).abs() / v64
        print(f"lpips vgg reference normalisation {h} x {w}: largest relative error {rel.max():.3e} = {rel.max() / worst_ref:.2f} x the largest feature e_ref")
        assert (rel <= 8 * worst_ref).all()
        assert torch.equal(m(a.to(DEV), a.to(DEV)).cpu(), torch.zeros(3, dtype=torch.float64)) and torch.equal(m(b.to(DEV), a.to(DEV)).cpu(), v)


@pytest.mark.parametrize("net", NETS)
def test_invariances(nets, spec, net):
    m = nets[net]
    a, b = (t.to(DEV) for t in spec[(net, 35, 37)][:2])
    v = m(a, b)
    assert torch.equal(m(a, a), torch.zeros(3, dtype=torch.float64, device=DEV))          # LPIPS(x, x) == 0.0
    assert torch.equal(m(b, a), v)                                                        # symmetric bit for bit
    assert torch.equal(m(a, b), v)                                                        # rerun
    for chunk in (1, 3):
        assert torch.equal(m(a, b, chunk=chunk), v)
    for i in range(3):
        assert torch.equal(m(a[i:i + 1], b[i:i + 1])[0], v[i]), i                         # alone
    order = torch.tensor([2, 0, 1], device=DEV)
    assert torch.equal(m(a[order], b[order]), v[order])                                   # another position
    assert torch.equal(m(a.bfloat16(), b.bfloat16()), m(a.bfloat16().float(), b.bfloat16().float()))
    s = m.min_size
    with pytest.raises(ValueError, match=f"at least {s} x {s}"):
        m(a[:, :, :s - 1, :s], b[:, :, :s - 1, :s])
    with torch.no_grad():                                                                 # the packs follow the parameters' versions
        m.lins()[-1].weight.mul_(2)
    assert not torch.equal(m(a, b), v)
    with torch.no_grad():
        m.lins()[-1].weight.mul_(0.5)
    assert torch.equal(m(a, b), v)


# ---- 6. the training loss's exact twin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 96, 128)])
def test_training_loss_against_its_exact_twin(shape):
    """dmvae_amd.utils.lpips.LPIPS (bf16 trunk, fused f32 reduction) against the exact-f32 trunk and f64 head in the reference's own normalisation, on the
    seeded weights, images and shapes of tests/test_gpu_lpips.py; 5e-3 relative, that file's tolerance for the value against its oracle."""
    from dmvae_amd.models.lpips_eval import LPIPSVGG
    from test_gpu_lpips import _lpips
    b, hh, ww = shape
    lp = _lpips()
    lp.net.trunk_loaded = True                                          # the seeded trunk stands in for a loaded one
    g = torch.Generator().manual_seed(1)
    img = torch.rand(b, 3, hh, ww, generator=g) * 2 - 1
    rec = (img + 0.3 * torch.randn(b, 3, hh, ww, generator=g)).clamp(-1, 1)
    lpd = lp.cuda()
    twin = LPIPSVGG.from_training(lpd, normalize="reference")
    assert next(twin.parameters()).is_cuda and twin.head_form == 1 and twin.eps == 1e-10
    with torch.no_grad():
        val = lpd(img.cuda(), rec.cuda()).item()
    want = twin(img.cuda(), rec.cuda()).mean().item()
    print(f"lpips twin {shape}: training loss (bf16) {val:.7e}, exact twin {want:.7e}, relative distance {abs(val - want) / want:.3e}")
    assert want > 0 and abs(val - want) <= 5e-3 * want


# ---- 7. the public interface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS)
def test_metrics_lpips_and_evaluate_on_device_tensors(nets, spec, monkeypatch, net):
    from dmvae_amd import metrics
    from dmvae_amd.evaluate import evaluate
    for var in ("DMVAE_LPIPS_ALEX_WEIGHTS", "DMVAE_LPIPS_VGG_WEIGHTS", "DMVAE_LPIPS_SQUEEZE_WEIGHTS"):
        monkeypatch.delenv(var, raising=False)
    m = nets[net]
    a, b = (t.to(DEV) for t in spec[(net, 64, 48)][:2])
    metrics.configure_lpips(m)
    try:
        got = metrics.LPIPS(a, b, net_type=net)
        assert got.dtype == torch.float32 and got.dim() == 0 and got.device == a.device
        assert torch.equal(got, m(a, b).mean().float()) and got.item() > 0
        assert metrics.LPIPS(a, a, net_type=net).item() == 0.0
        with pytest.raises(ValueError, match=r"\[-1, 1\]"):
            metrics.LPIPS(a * 1.5, b, net_type=net)
        with pytest.raises(NotImplementedError, match="AlexNet"):
            metrics.LPIPS(a, b)                                          # one network per type: 'alex' is still unconfigured
    finally:
        metrics.configure_lpips(None)
    with pytest.raises(NotImplementedError, match="not built"):
        metrics.LPIPS(a, b, net_type=net)

    class StubVAE(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1))

        def encode(self, x):
            return x * 0.5

        def decode(self, z):
            return z * 2.6

    imgs = torch.cat(spec[(net, 64, 48)][:2])
    batches = [(t, torch.zeros(len(t), dtype=torch.long)) for t in imgs.split([1, 3, 2])]
    plain = evaluate(StubVAE().to(DEV), batches, num_samples=8, device=DEV)
    with_lpips = evaluate(StubVAE().to(DEV), batches, num_samples=8, device=DEV, lpips=m)
    assert "LPIPS" not in plain and set(with_lpips) == set(plain) | {"LPIPS"} and all(with_lpips[k] == plain[k] for k in plain)
    want = m((imgs * 1.3).clamp(-1, 1).to(DEV), imgs.to(DEV)).sum().item() / 8
    assert want > 0 and abs(with_lpips["LPIPS"] - want) <= 1e-14 * want                   # the same per-image bits, added batch by batch
