"""GPU: the kernels of csrc/inception.hip against f64 CPU references with derived bounds, and dmvae_amd.models.inception.InceptionV3Compat against the f64
specification of tests/inception_spec.py with seeded random parameters (the published weights are on no machine this package is developed on).

Bounds.  A convolution output is one k-ordered chain of K fmaf from 0 and one more fmaf for scale / shift, so by the standard running-error bound
|err| <= gamma_{K+2} (sum_k |a_k w_k| |scale| + |shift|), gamma_n = n u / (1 - n u), u = 2^-24; on small integers every partial sum is exact.  The whole
network is held to e_hip <= 8 e_ref per image, e_ref being the stock f32 CPU composition's error against the same f64 values, computed in the same run.

Measured on an MI355X (profiles/inception_accuracy.txt): e_hip / e_ref is 1.5 - 1.7 (features) and 1.9 (logits_unbiased) at 299, 2.0 - 2.2 and
2.0 - 2.5 at 139 -- e_hip 3.0e-7 ... 1.0e-6, above e_ref for every image and inside the margin; every conv form stays within 0.21 of its bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SENTINEL = -7.7725e5


def gamma(n):
    return n * U / (1 - n * U)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# (kh, kw), stride, (ph, pw): every form of include/dmvae_hip.h's dmvae_conv2d_f32_fwd
FORMS = [((1, 1), 1, (0, 0)), ((3, 3), 1, (0, 0)), ((3, 3), 2, (0, 0)), ((3, 3), 1, (1, 1)), ((5, 5), 1, (2, 2)), ((1, 7), 1, (0, 3)), ((7, 1), 1, (3, 0)),
         ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0))]


def run_conv(x, w, kernel, stride, pad, scale, shift, relu, off, extra_c, extra_rows=5):
    """x NCHW f32, w OIHW f32 (CPU) -> (the kernel's [B, Ho, Wo, cout] slice, the whole sentinel-filled buffer as [rows, pitch], M)."""
    from dmvae_amd import ops
    cout = w.shape[0]
    ho, wo = (x.shape[2] + 2 * pad[0] - kernel[0]) // stride + 1, (x.shape[3] + 2 * pad[1] - kernel[1]) // stride + 1
    m, pitch = x.shape[0] * ho * wo, off + cout + extra_c
    buf = torch.full((m + extra_rows, pitch), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[:m].view(x.shape[0], ho, wo, pitch)
    dv = lambda t: None if t is None else t.to(DEV)
    ops.conv2d_f32(nhwc(x).to(DEV), ops.pack_conv_weight_f32(w).to(DEV), kernel, stride, pad, dv(scale), dv(shift), relu, out, off)
    torch.cuda.synchronize()
    return buf[:m, off:off + cout].cpu().view(x.shape[0], ho, wo, cout), buf.cpu(), m


def assert_untouched(buf, m, off, cout):
    s = torch.tensor(SENTINEL, dtype=torch.float32)
    assert torch.equal(buf[:m, :off], s.expand(m, off)) and torch.equal(buf[:m, off + cout:], s.expand(m, buf.shape[1] - off - cout))
    assert torch.equal(buf[m:], s.expand(buf.shape[0] - m, buf.shape[1]))


def check_conv(b, h, w_, cin, cout, kernel, stride, pad, seed):
    g = torch.Generator().manual_seed(seed)
    x, w = torch.randn(b, cin, h, w_, generator=g), torch.randn(cout, cin, *kernel, generator=g) / (cin * kernel[0] * kernel[1]) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    k = cin * kernel[0] * kernel[1]
    acc = F.conv2d(x.double(), w.double(), None, stride, pad)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, stride, pad)
    ref = acc * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    bound = gamma(k + 2) * (mag * scale.double().view(1, -1, 1, 1) + shift.double().abs().view(1, -1, 1, 1))
    for relu in (False, True):
        got, buf, m = run_conv(x, w, kernel, stride, pad, scale, shift, relu, 16, 12)
        assert m % 64 != 0
        want = nhwc(ref.clamp_min(0) if relu else ref)
        err = (got.double() - want).abs()
        worst = (err / nhwc(bound)).max().item()
        print(f"conv {kernel} s{stride} p{pad} cin {cin} cout {cout} relu {relu}: max err / bound {worst:.3f}")
        assert worst <= 1.0                                           # ReLU is 1-Lipschitz: the bound carries over
        assert_untouched(buf, m, 16, cout)
    # small integers, no scale / shift: every product and partial sum is an integer below 2^24 -- equality
    xi = torch.randint(-4, 5, x.shape, generator=g).float()
    wi = torch.randint(-4, 5, w.shape, generator=g).float()
    got, buf, m = run_conv(xi, wi, kernel, stride, pad, None, None, False, 4, 0)
    assert torch.equal(got.double(), nhwc(F.conv2d(xi.double(), wi.double(), None, stride, pad)))
    assert_untouched(buf, m, 4, cout)


@pytest.mark.parametrize("kernel,stride,pad", FORMS)
def test_conv_forms(kernel, stride, pad):
    for i, (cin, cout) in enumerate((ci, co) for ci in (16, 48, 80) for co in (16, 80)):
        check_conv(2, 9, 11, cin, cout, kernel, stride, pad, 100 + i)


def test_conv_first_layer_cin3():
    check_conv(2, 9, 11, 3, 16, (3, 3), 2, (0, 0), 7)
    check_conv(2, 9, 11, 3, 80, (3, 3), 2, (0, 0), 8)
    check_conv(3, 23, 21, 3, 32, (3, 3), 2, (0, 0), 9)               # M = 330: six tiles, the last ragged


def test_conv_fc_form():
    check_conv(2, 1, 1, 2048, 1008, (1, 1), 1, (0, 0), 11)
    check_conv(5, 1, 1, 80, 1008, (1, 1), 1, (0, 0), 12)


@pytest.mark.parametrize("h,w_", [(9, 11), (7, 7)])
@pytest.mark.parametrize("c", [16, 80])
def test_pools(h, w_, c):
    from dmvae_amd import ops
    g = torch.Generator().manual_seed(h * 100 + c)
    x = torch.randn(2, c, h, w_, generator=g)
    xd = nhwc(x).to(DEV)

    def run(t, mode):
        ho, wo = ((h - 3) // 2 + 1, (w_ - 3) // 2 + 1) if mode == ops.POOL_MAX_S2 else (h, w_)
        m = 2 * ho * wo
        buf = torch.full((m + 3, c + 24), SENTINEL, dtype=torch.float32, device=DEV)
        ops.pool2d_f32(t, mode, buf[:m].view(2, ho, wo, c + 24), 8)
        out = buf.cpu()
        assert_untouched(out, m, 8, c)
        return out[:m, 8:8 + c].view(2, ho, wo, c)
    assert torch.equal(run(xd, ops.POOL_MAX_S2), nhwc(F.max_pool2d(x, 3, 2)))
    assert torch.equal(run(xd, ops.POOL_MAX_S1P1), nhwc(F.max_pool2d(x, 3, 1, 1)))
    neg = -x.abs() - 1
    got = run(nhwc(neg).to(DEV), ops.POOL_MAX_S1P1)
    assert (got < 0).all() and torch.equal(got, nhwc(F.max_pool2d(neg, 3, 1, 1)))      # the zero padding is no candidate
    # average: the f32 raster-order sum of n <= 9 terms (error <= (n - 1) u sum|x| to first order) and one division: 10 u sum|x| / count
    ref = F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False)
    bound = 10 * U * F.avg_pool2d(x.double().abs(), 3, 1, 1, count_include_pad=False)   # = 10 u sum|x| / count
    got = run(xd, ops.POOL_AVG_S1P1)
    assert ((got.double() - nhwc(ref)).abs() <= nhwc(bound)).all()
    xi = (torch.randint(-8, 9, x.shape, generator=g) * 36).float()                      # window sums divide by 4, 6 and 9
    assert torch.equal(run(nhwc(xi).to(DEV), ops.POOL_AVG_S1P1).double(), nhwc(F.avg_pool2d(xi.double(), 3, 1, 1, count_include_pad=False)))
    # global average: rand's values are multiples of 2^-24 in [0, 1), so the f64 sum of h w of them is exact in any order
    xr = torch.rand(2, h, w_, c, generator=g)
    assert torch.equal(ops.global_avgpool_f32(xr.to(DEV)).cpu(), (xr.double().sum(dim=(1, 2)) / (h * w_)).float())


def test_input_kernel():
    from dmvae_amd import ops
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (3, 3, 13, 9), generator=g, dtype=torch.uint8)
    want = nhwc((u8.float() - 128) / 128)
    assert torch.equal(ops.inception_input(u8.to(DEV)).cpu(), want)
    assert torch.equal(ops.inception_input(nchw(want).to(DEV)).cpu(), want)              # f32: already normalised, layout only
    full = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).expand(1, 3, 16, 16).contiguous()
    assert torch.equal(ops.inception_input(full.to(DEV)).cpu(), nhwc((full.float() - 128) / 128))


# ---- the whole network ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return S.random_state_dict(0)


@pytest.fixture(scope="module")
def net(sd):
    from dmvae_amd.models.inception import InceptionV3Compat
    n = InceptionV3Compat()
    n.load_state_dict(sd)
    return n.to(DEV)


@pytest.fixture(scope="module")
def spec(sd):
    """size -> (uint8 images, f64 features, f64 logits_unbiased, f64 logits, e_ref features [B], e_ref logits_unbiased [B]); computed once, never modified."""
    out = {}
    for n, size in ((2, 299), (5, 139)):
        u8 = S.images(n, size)
        f, lu, l = S.forward(sd, S.normalise(u8))
        f32, lu32, _ = S.forward(sd, S.normalise(u8).float(), torch.float32)
        out[size] = (u8, f, lu, l, S.rel_l2(f32, f), S.rel_l2(lu32, lu))
    return out


@pytest.mark.parametrize("size", [299, 139])
def test_whole_network_against_the_f64_specification(net, spec, size):
    """Per image: e_hip <= 8 e_ref for the features and for logits_unbiased; logits = logits_unbiased + bias to one rounding."""
    u8, f64, lu64, l64, eref_f, eref_l = spec[size]
    share, lo, hi = S.check_alive(f64)
    assert share >= 0.5 and 1e-3 <= lo and hi <= 1e3
    x = S.normalise(u8).float().to(DEV)
    f, lu = net.features_logits(x)
    _, lb = net.features_logits(x, biased=True)
    e_f, e_l = S.rel_l2(f, f64), S.rel_l2(lu, lu64)
    for i in range(len(u8)):
        print(f"inception accuracy size {size} image {i}: features e_hip {e_f[i]:.3e} e_ref {eref_f[i]:.3e} ratio {e_f[i] / eref_f[i]:.2f}; "
              f"logits_unbiased e_hip {e_l[i]:.3e} e_ref {eref_l[i]:.3e} ratio {e_l[i] / eref_l[i]:.2f}")
    assert (e_f <= 8 * eref_f).all() and (e_l <= 8 * eref_l).all()
    assert torch.equal(lb.cpu(), lu.cpu() + net.fc.bias.cpu())                           # one f32 addition of the bias
    if size == 299:
        assert torch.equal(net(u8.to(DEV)), f)                                           # forward(u8) normalises in the input kernel: the same bits


def test_invariance_batch_position_rerun_and_chunks(net, spec):
    u8 = spec[139][0]
    x = S.normalise(u8).float().to(DEV)
    f5, l5 = net.features_logits(x)
    for i in range(5):
        f1, l1 = net.features_logits(x[i:i + 1].contiguous())
        assert torch.equal(f1[0], f5[i]) and torch.equal(l1[0], l5[i]), i
    f5b, l5b = net.features_logits(x)
    assert torch.equal(f5b, f5) and torch.equal(l5b, l5)
    fc, lc = net.features_logits(x, chunk=2)
    assert torch.equal(fc, f5) and torch.equal(lc, l5)
    assert torch.equal(net(u8.to(DEV), chunk=2), net(u8.to(DEV)))                        # through the 139 -> 299 resize as well


def test_fid_and_fidelity_metrics_plumbing(net, tmp_path):
    from dmvae_amd import ops
    from dmvae_amd.fid import FID
    from dmvae_amd.fidelity import FidelityMetrics
    g = torch.Generator().manual_seed(5)
    img01 = torch.rand(4, 3, 64, 64, generator=g).to(DEV)
    a, b = FID(feature=net).to(DEV), FID(feature=net).to(DEV)
    a.update(img01, real=True)
    b.update_features(net(ops.fid_resize_u8(img01, 299)), real=True)
    for k in ("sum", "cov_sum", "num_samples"):
        assert torch.equal(getattr(a, f"real_features_{k}"), getattr(b, f"real_features_{k}"))
    assert a.real_features_num_samples.item() == 4 and a.real_features_sum.abs().sum().item() > 0

    u8 = torch.randint(0, 256, (8, 32, 32, 3), generator=g, dtype=torch.uint8).to(DEV)
    m1, m2 = (FidelityMetrics(net.extractor(), num_features=2048).to(DEV) for _ in range(2))
    m1.update_uint8(u8)
    m2.update_features(*net.features_logits(ops.resize_tf1_bilinear(u8, 299)))
    assert torch.equal(m1.features_sum, m2.features_sum) and torch.equal(m1.features_cov_sum, m2.features_cov_sum) and m1.num_samples == m2.num_samples == 8
    lo = torch.randn(2048, 32, generator=g, dtype=torch.float64)
    np.savez(tmp_path / "stats.npz", mu=torch.randn(2048, generator=g, dtype=torch.float64).numpy(), sigma=(lo @ lo.t() / 32 + 0.1 * torch.eye(2048)).numpy())
    m1.load_statistics_file(tmp_path / "stats.npz")
    out = m1.compute(splits=2)
    assert set(out) == {"inception_score_mean", "inception_score_std", "frechet_inception_distance"}
    assert all(np.isfinite(v) for v in out.values()), out


def test_packs_follow_parameter_versions(sd):
    """An in-place update that moves the parameter's `_version` (what load_state_dict and every in-place op under no_grad do) is seen by the next call.
    A write through `.data` is NOT such an update -- torch gives `.data` a version counter of its own, so `p.data.mul_(2)` leaves `p._version` where it
    was and no cache keyed on versions can see it -- which is why this test multiplies under no_grad, and why the module has `refresh()`."""
    from dmvae_amd.models.inception import InceptionV3Compat
    net = InceptionV3Compat()
    net.load_state_dict(sd)
    net = net.to(DEV)
    x = S.normalise(S.images(1, 75)).float().to(DEV)
    f0, _ = net.features_logits(x)
    p = net.Mixed_6b.branch7x7_2.conv.weight
    with torch.no_grad():
        p.mul_(2)
    f1, _ = net.features_logits(x)
    assert not torch.equal(f1, f0)
    v = p._version
    p.data.mul_(0.5)
    assert p._version == v
    net.refresh()
    assert torch.equal(net.features_logits(x)[0], f0)                                    # * 2 then * 0.5: the original bits
    net.load_state_dict(S.random_state_dict(1))
    assert not torch.equal(net.features_logits(x)[0], f0)
