"""GPU: the evaluation LPIPS (evaluation/metrics.py:26-29) -- the (11, 11) stride 4 padding 2 form of dmvae_conv2d_f32_fwd, the input pass and the f64 head
of csrc/lpips_eval.hip against CPU references with derived bounds, and dmvae_amd.models.lpips_alex.LPIPSAlex against the f64 specification of
tests/lpips_eval_spec.py with seeded random parameters (neither the library nor a weight file is on any machine this package is developed on).

Bounds.
  Convolution: an output is one k-ordered chain of K = 363 fmaf from 0 and one more fmaf for scale / shift, so by the standard running-error bound
|err| <= gamma_{K+2} (sum_k |a_k w_k| |scale| + |shift|), gamma_n = n u / (1 - n u), u = 2^-24; on small integers every partial sum is exact.
  Head (u = 2^-53; every element is widened to f64 exactly, and the square of an f32 is exact in f64).  Per pixel and side, s = sum_c f_c^2 carries only
its additions' error, <= gamma_c s whatever the order; eps + s, the root, the reciprocal and the product f r add one rounding each, so the computed
n^ = n (1 + t) with |t| <= k := gamma_{c+5}.  The computed difference d^ = fl(n1^ - n2^) is off by at most E = (k (|n1| + |n2|) + u |d|)(1 + u) -- an
ABSOLUTE error: where n1 and n2 nearly cancel it does not shrink with d.  Squaring and weighting add two roundings: the computed term w d^2 is off by at most
T = |w| (2 |d| E + E^2 + 2 u d^2).  The terms are then added over the channels of a pixel, the pixels of a workgroup, the workgroups of a pair: any path
through those sums is shorter than c + h w + 32 additions, which costs gamma_{c + h w + 32} sum |w| d^2 (for lin >= 0 the terms are non-negative; for signed
lin the bound holds with sum |w| as written).  The division by h w and the optional addition to `out` are one rounding each of the result.  So
  |err| <= B := (sum_{pixels, c} T + gamma_{c + h w + 32} sum |w| d^2) / (h w) + 2 u |v|,
taken 1.01 times for the second-order terms dropped above.  The numpy f64 evaluation it is compared with obeys the same bound (its sums are pairwise, its
n a single division): the test holds |kernel - numpy| <= 2.02 B.
  Whole network: per tap and image, the rel-L2 error of the f32 features against the f64 specification is held to 8 e_ref, e_ref being the stock f32 CPU
composition's error against the same f64 values, computed in the same run; the per-image value's relative error to 8 x the largest feature e_ref of the
run (the value's own f32 error is no yardstick: by cancellation it ranges over more than a decade from image to image).

Measured on an MI355X (profiles/lpips_eval_accuracy.txt): e_hip / e_ref is 1.00 at tap 0, 1.5 - 1.6 at tap 1, 1.8 - 2.2 at tap 2, 2.1 - 2.4 at
tap 3 and 2.2 - 2.7 at tap 4 (e_hip 3.3e-7 ... 1.3e-6, e_ref 3.3e-7 ... 5.7e-7) -- at or above e_ref for every image and inside the margin; the values'
relative errors are 9e-10 ... 1.9e-7, at most 0.34 x the largest feature e_ref; the (11, 11) form stays within 0.012 of its bound and the head within 0.002
of 2 B (B / |v| is 7e-14 ... 9e-13 for lin >= 0)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_eval_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
U64 = 2.0 ** -53
SENTINEL = -7.7725e5


def gamma(n, u=U):
    return n * u / (1 - n * u)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---- 1. the (11, 11) / stride 4 / padding (2, 2) form ---------------------------------------------------------------------------------------------
KERNEL, STRIDE, PAD = (11, 11), 4, (2, 2)


def run_conv(x, w, scale, shift, relu, off, extra_c, extra_rows=5):
    """x NCHW f32, w OIHW f32 (CPU) -> (the kernel's [B, Ho, Wo, cout] slice, the whole sentinel-filled buffer as [rows, pitch], M)."""
    from dmvae_amd import ops
    cout = w.shape[0]
    ho, wo = (x.shape[2] + 2 * PAD[0] - KERNEL[0]) // STRIDE + 1, (x.shape[3] + 2 * PAD[1] - KERNEL[1]) // STRIDE + 1
    m, pitch = x.shape[0] * ho * wo, off + cout + extra_c
    buf = torch.full((m + extra_rows, pitch), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[:m].view(x.shape[0], ho, wo, pitch)
    dv = lambda t: None if t is None else t.to(DEV)
    packed = ops.pack_conv_weight_f32(w)
    assert tuple(packed.shape) == (31, cout, 16)                     # 121 taps in 31 chunks of four
    ops.conv2d_f32(nhwc(x).to(DEV), packed.to(DEV), KERNEL, STRIDE, PAD, dv(scale), dv(shift), relu, out, off)
    torch.cuda.synchronize()
    return buf[:m, off:off + cout].cpu().view(x.shape[0], ho, wo, cout), buf.cpu(), m


def assert_untouched(buf, m, off, cout):
    s = torch.tensor(SENTINEL, dtype=torch.float32)
    assert torch.equal(buf[:m, :off], s.expand(m, off)) and torch.equal(buf[:m, off + cout:], s.expand(m, buf.shape[1] - off - cout))
    assert torch.equal(buf[m:], s.expand(buf.shape[0] - m, buf.shape[1]))


@pytest.mark.parametrize("b,h,w_", [(2, 23, 27), (3, 63, 47)])
@pytest.mark.parametrize("cout", [16, 64, 80])
def test_conv_11x11_stride4_pad2(b, h, w_, cout):
    """M = 60 (one ragged tile) and M = 495 (eight tiles, the last ragged); 31 chunks are seven full stages and one of three chunks, the last chunk one tap."""
    g = torch.Generator().manual_seed(1000 + cout + h)
    x, w = torch.randn(b, 3, h, w_, generator=g), torch.randn(cout, 3, *KERNEL, generator=g) / 363 ** 0.5
    k = 363
    acc = F.conv2d(x.double(), w.double(), None, STRIDE, PAD)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, STRIDE, PAD)
    for with_scale in (True, False):                                   # False: scale = NULL, shift = the bias -- the form AlexNet's layers use
        scale = torch.rand(cout, generator=g) + 0.5 if with_scale else None
        shift = torch.randn(cout, generator=g)
        sc = (scale.double() if with_scale else torch.ones(cout, dtype=torch.float64)).view(1, -1, 1, 1)
        ref = acc * sc + shift.double().view(1, -1, 1, 1)
        bound = gamma(k + 2) * (mag * sc + shift.double().abs().view(1, -1, 1, 1))
        for relu in (False, True):
            got, buf, m = run_conv(x, w, scale, shift, relu, 16, 12)
            assert m % 64 != 0
            want = nhwc(ref.clamp_min(0) if relu else ref)
            err = (got.double() - want).abs()
            worst = (err / nhwc(bound)).max().item()
            print(f"conv (11, 11) s4 p2 {b}x{h}x{w_} cout {cout} scale {with_scale} relu {relu}: max err / bound {worst:.3f}")
            assert worst <= 1.0                                        # ReLU is 1-Lipschitz: the bound carries over
            assert_untouched(buf, m, 16, cout)
    # small integers, no scale / shift: every product and partial sum is an integer below 2^24 -- equality
    xi = torch.randint(-4, 5, x.shape, generator=g).float()
    wi = torch.randint(-4, 5, w.shape, generator=g).float()
    got, buf, m = run_conv(xi, wi, None, None, False, 4, 0)
    assert torch.equal(got.double(), nhwc(F.conv2d(xi.double(), wi.double(), None, STRIDE, PAD)))
    assert_untouched(buf, m, 4, cout)


# ---- 2. the input pass --------------------------------------------------------------------------------------------------------------------------
def test_input_pass_is_the_torch_expression_bit_for_bit():
    from dmvae_amd import ops
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(3, 3, 13, 9, generator=g) * 2 - 1, torch.rand(3, 3, 13, 9, generator=g) * 2 - 1
    a[0, :, 0, 0], a[0, :, 0, 1], b[1, :, 2, 2] = -1.0, 1.0, 0.0
    shift, scale = torch.tensor(S.SHIFT).view(1, 3, 1, 1), torch.tensor(S.SCALE).view(1, 3, 1, 1)
    for cast in (lambda t: t, lambda t: t.bfloat16()):
        xa, xb = cast(a), cast(b)
        want = torch.cat([nhwc((xa.float() - shift) / scale), nhwc((xb.float() - shift) / scale)])      # rows 0 .. B the first image, B .. 2 B the second
        got = ops.lpips_input(xa.to(DEV), xb.to(DEV))
        assert got.dtype == torch.float32 and tuple(got.shape) == (6, 13, 9, 3)
        assert torch.equal(got.cpu(), want)
    assert not torch.equal(got[:3], got[3:])


# ---- 3. the head --------------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(3, 15, 15, 64), (2, 7, 7, 192), (2, 5, 3, 384), (1, 1, 1, 256), (70, 3, 11, 64), (2, 4, 4, 1024)]


def head_inputs(pairs, h, w, c, seed, signed=False):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(2 * pairs, h, w, c, generator=g).clamp_min(0)                      # what a ReLU leaves
    f[pairs:] = (f[:pairs] + 0.3 * torch.randn(pairs, h, w, c, generator=g)).clamp_min(0)
    lin = torch.rand(c, generator=g) / c
    if signed:
        lin = lin * (torch.randint(0, 2, (c,), generator=g) * 2 - 1).float()
    return f, lin


def head_reference(f, lin, eps):
    """numpy f64 -> (values [pairs], the bound B of this file's docstring [pairs])."""
    x = f.numpy().astype(np.float64)
    pairs, (h, w, c) = x.shape[0] // 2, x.shape[1:]
    wl = lin.numpy().astype(np.float64)
    n1 = x[:pairs] / np.sqrt(eps + (x[:pairs] * x[:pairs]).sum(-1, keepdims=True))
    n2 = x[pairs:] / np.sqrt(eps + (x[pairs:] * x[pairs:]).sum(-1, keepdims=True))
    d = n1 - n2
    v = ((d * d) * wl).sum(-1).mean(axis=(1, 2))
    k = gamma(c + 5, U64)
    e = (k * (np.abs(n1) + np.abs(n2)) + U64 * np.abs(d)) * (1 + U64)
    t = np.abs(wl) * (2 * np.abs(d) * e + e * e + 2 * U64 * d * d)
    bound = (t.sum(axis=(1, 2, 3)) + gamma(c + h * w + 32, U64) * (np.abs(wl) * d * d).sum(axis=(1, 2, 3))) / (h * w) + 2 * U64 * np.abs(v)
    return torch.from_numpy(v), torch.from_numpy(1.01 * bound)


@pytest.mark.parametrize("pairs,h,w,c", HEAD_SHAPES)
@pytest.mark.parametrize("signed", [False, True])
def test_head_against_f64_numpy(pairs, h, w, c, signed):
    from dmvae_amd import ops
    f, lin = head_inputs(pairs, h, w, c, 7 * c + h + signed, signed)
    want, bound = head_reference(f, lin, 1e-8)
    got = ops.lpips_head(f.to(DEV), lin.to(DEV), 1e-8).cpu()
    assert got.dtype == torch.float64 and tuple(got.shape) == (pairs,)
    ratio = ((got - want).abs() / (2 * bound)).max().item()
    print(f"lpips head {pairs} x {h} x {w} x {c} signed {signed}: value {want[0].item():+.6e}, max |err| / (2 B) {ratio:.3f}, "
          f"B / |v| {(bound / want.abs()).max().item():.2e}")
    assert ratio <= 1.0
    if not signed:
        assert (got > 0).all()
    e6 = ops.lpips_head(f.to(DEV), lin.to(DEV), 1e-6).cpu()                              # eps is an argument
    want6, bound6 = head_reference(f, lin, 1e-6)
    assert ((e6 - want6).abs() <= 2 * bound6).all() and not torch.equal(e6, got)


@pytest.mark.parametrize("pairs,h,w,c", HEAD_SHAPES)
def test_head_identities(pairs, h, w, c):
    from dmvae_amd import ops
    f, lin = head_inputs(pairs, h, w, c, 11 * c + w)
    fd, ld = f.to(DEV), lin.to(DEV)
    v = ops.lpips_head(fd, ld)
    # identical halves: exactly 0.0; swapped halves: the same bits
    same = torch.cat([fd[:pairs], fd[:pairs]])
    assert torch.equal(ops.lpips_head(same, ld), torch.zeros(pairs, dtype=torch.float64, device=DEV))
    assert torch.equal(ops.lpips_head(torch.cat([fd[pairs:], fd[:pairs]]), ld), v)
    # a pixel whose channels are all zero on both sides adds 0, not NaN; all-zero images give 0.0
    z = f.clone()
    z[:, 0, 0, :] = 0
    want, bound = head_reference(z, lin, 1e-8)
    got = ops.lpips_head(z.to(DEV), ld).cpu()
    assert torch.isfinite(got).all() and ((got - want).abs() <= 2 * bound).all()
    assert torch.equal(ops.lpips_head(torch.zeros_like(fd), ld).cpu(), torch.zeros(pairs, dtype=torch.float64))
    # accumulate adds the level's value to out once; memory around out is untouched
    buf = torch.full((pairs + 4,), float(SENTINEL), dtype=torch.float64, device=DEV)
    out = buf[2:2 + pairs]
    assert ops.lpips_head(fd, ld, out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out, v) and (buf[:2] == SENTINEL).all() and (buf[2 + pairs:] == SENTINEL).all()
    start = torch.arange(pairs, dtype=torch.float64, device=DEV) * 0.37 + 1.25
    out.copy_(start)
    ops.lpips_head(fd, ld, out=out, accumulate=True)
    assert torch.equal(out, start + v) and (buf[:2] == SENTINEL).all() and (buf[2 + pairs:] == SENTINEL).all()
    # the same bits on a rerun, alone, and at another position of a larger batch
    assert torch.equal(ops.lpips_head(fd, ld), v)
    for i in sorted({0, pairs // 2, pairs - 1}):
        alone = torch.cat([fd[i:i + 1], fd[pairs + i:pairs + i + 1]])
        assert torch.equal(ops.lpips_head(alone, ld)[0], v[i]), i
    order = torch.arange(pairs - 1, -1, -1, device=DEV)
    pad = torch.rand(3, h, w, c, device=DEV)
    moved = torch.cat([pad, fd[:pairs][order], pad.flip(0), fd[pairs:][order]])
    assert torch.equal(ops.lpips_head(moved, ld)[3:], v[order])


# ---- 4. - 6. the whole network ------------------------------------------------------------------------------------------------------------------
SIZES = [(64, 64), (95, 71)]


@pytest.fixture(scope="module")
def sd():
    return S.random_state_dict(0)


@pytest.fixture(scope="module")
def net(sd):
    from dmvae_amd.models.lpips_alex import LPIPSAlex
    n = LPIPSAlex()
    n.load_state_dict(sd)
    return n.to(DEV)


@pytest.fixture(scope="module")
def spec(sd):
    """(h, w) -> (a, b, f64 values [4], f64 taps of both images, e_ref per tap [2 x 4] each); computed once, never modified."""
    out = {}
    for h, w in SIZES:
        a, b = S.image_pairs(4, h, w)
        v, t1, t2 = S.forward(sd, a, b)
        _, s1, s2 = S.forward(sd, a, b, torch.float32)
        taps = [torch.cat([x, y]) for x, y in zip(t1, t2)]
        eref = [S.rel_l2(torch.cat([x, y]), t) for x, y, t in zip(s1, s2, taps)]
        assert S.check_alive(v, t1, t2)[0] >= 0.25 and (v > 0).all() and torch.isfinite(v).all()
        out[(h, w)] = (a, b, v, taps, eref)
    return out


@pytest.mark.parametrize("h,w", SIZES)
def test_whole_network_against_the_f64_specification(net, spec, h, w):
    """Per tap and image e_hip <= 8 e_ref; per image the value's relative error <= 8 max e_ref.  Measured on an MI355X (profiles/lpips_eval_accuracy.txt):
    feature ratios 1.00 - 2.67, value errors at most 0.34 x the largest feature e_ref."""
    a, b, v64, taps64, eref = spec[(h, w)]
    taps = net.taps(a.to(DEV), b.to(DEV))
    worst_ref = max(e.max().item() for e in eref)
    for level, (f, f64, e_ref) in enumerate(zip(taps, taps64, eref)):
        assert tuple(f.shape) == (8, f64.shape[2], f64.shape[3], f64.shape[1])
        e_hip = S.rel_l2(nchw(f), f64)
        for i in range(8):
            print(f"lpips accuracy {h} x {w} tap {level} image {'ab'[i // 4]}{i % 4}: e_hip {e_hip[i]:.3e} e_ref {e_ref[i]:.3e} ratio {e_hip[i] / e_ref[i]:.2f}")
        assert (e_hip <= 8 * e_ref).all(), level
    v = net(a.to(DEV), b.to(DEV)).cpu()
    assert v.dtype == torch.float64 and tuple(v.shape) == (4,)
    rel = (v - v64).abs() / v64
    for i in range(4):
        print(f"lpips accuracy {h} x {w} value {i}: {v[i].item():.9e} (f64 {v64[i].item():.9e}) relative error {rel[i]:.3e} = {rel[i] / worst_ref:.2f} x the "
              f"largest feature e_ref {worst_ref:.3e}")
    assert (rel <= 8 * worst_ref).all()


def test_invariances(net, spec):
    a, b = (t.to(DEV) for t in spec[(95, 71)][:2])
    v = net(a, b)
    assert torch.equal(net(a, a), torch.zeros(4, dtype=torch.float64, device=DEV))        # LPIPS(x, x) == 0.0
    assert torch.equal(net(b, a), v)                                                      # symmetric bit for bit
    assert torch.equal(net(a, b), v)                                                      # rerun
    for chunk in (1, 3):
        assert torch.equal(net(a, b, chunk=chunk), v)
    for i in range(4):
        assert torch.equal(net(a[i:i + 1], b[i:i + 1])[0], v[i]), i                       # alone
    order = torch.tensor([2, 0, 3, 1], device=DEV)
    assert torch.equal(net(a[order], b[order]), v[order])                                 # another position
    assert torch.equal(net(a.bfloat16(), b.bfloat16()), net(a.bfloat16().float(), b.bfloat16().float()))


def test_packs_follow_parameter_versions(sd, spec):
    """An in-place update under no_grad moves the parameter's `_version` and is seen by the next call; a write through `.data` moves none (torch gives
    `.data` a counter of its own) and is seen after `refresh()`."""
    from dmvae_amd.models.lpips_alex import LPIPSAlex
    net = LPIPSAlex()
    net.load_state_dict(sd)
    net = net.to(DEV)
    a, b = (t[:1].to(DEV) for t in spec[(64, 64)][:2])
    v0 = net(a, b)
    p = net.convs()[2].weight
    assert p is getattr(net.net.slice3, "6").weight
    with torch.no_grad():
        p.mul_(2)
    v1 = net(a, b)
    assert not torch.equal(v1, v0)
    ver = p._version
    p.data.mul_(0.5)
    assert p._version == ver and torch.equal(net(a, b), v1)                                # not seen: the packs are keyed on versions
    net.refresh()
    assert torch.equal(net(a, b), v0)                                                      # * 2 then * 0.5: the original bits
    with torch.no_grad():
        net.lins()[4].weight.mul_(3)
    assert not torch.equal(net(a, b), v0)
    net.load_state_dict(S.random_state_dict(1))
    assert not torch.equal(net(a, b), v0)


def test_metrics_lpips_and_evaluate_on_device_tensors(net, spec, monkeypatch):
    from dmvae_amd import metrics
    from dmvae_amd.evaluate import evaluate
    monkeypatch.delenv("DMVAE_LPIPS_ALEX_WEIGHTS", raising=False)
    a, b = (t.to(DEV) for t in spec[(64, 64)][:2])
    metrics.configure_lpips(net)
    try:
        got = metrics.LPIPS(a, b)
        assert got.dtype == torch.float32 and got.dim() == 0 and got.device == a.device
        assert torch.equal(got, net(a, b).mean().float())
        assert metrics.LPIPS(a, a).item() == 0.0
        with pytest.raises(ValueError, match=r"\[-1, 1\]"):
            metrics.LPIPS(a * 1.5, b)
    finally:
        metrics.configure_lpips(None)
    with pytest.raises(NotImplementedError, match="AlexNet"):
        metrics.LPIPS(a, b)

    class StubVAE(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1))

        def encode(self, x):
            return x * 0.5

        def decode(self, z):
            return z * 2.6

    imgs = torch.cat([spec[(64, 64)][0], spec[(64, 64)][1][:2]])
    batches = [(t, torch.zeros(len(t), dtype=torch.long)) for t in imgs.split([1, 3, 2])]
    plain = evaluate(StubVAE().to(DEV), batches, num_samples=8, device=DEV)
    with_lpips = evaluate(StubVAE().to(DEV), batches, num_samples=8, device=DEV, lpips=net)
    assert "LPIPS" not in plain and set(with_lpips) == set(plain) | {"LPIPS"} and all(with_lpips[k] == plain[k] for k in plain)
    want = net((imgs * 1.3).clamp(-1, 1).to(DEV), imgs.to(DEV)).sum().item() / 8
    assert want > 0 and abs(with_lpips["LPIPS"] - want) <= 1e-14 * want                   # the same per-image bits, added batch by batch
