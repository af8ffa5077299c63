"""FID on the MI355X (-m gpu): the f64 statistics kernel against X^T X in f64 on the CPU under the bound any summation order meets, the resize + quantise
kernel against the formula of tests/fid_spec.py at every pixel that does not hang on the last bits, and dmvae_amd.fid.FID end to end around a stub extractor,
alone and as `evaluate(..., fid=...)`'s metric."""
import pytest
import torch

import fid_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _x(n, f, dtype, seed=0, rows=None, ld=None, fill=float("nan")):
    """Features [n, f] as a view of a [rows, ld] buffer whose other elements are `fill`."""
    g = torch.Generator().manual_seed(1000 * n + f + seed)
    x = (torch.randn(n, f, generator=g) * 1.5 + 0.25).to(dtype)
    buf = torch.full((rows or n, ld or f), fill, dtype=dtype)
    buf[:n, :f] = x
    return x, buf.to(DEV)[:n, :f]


def _states(f):
    return torch.zeros(f, dtype=torch.float64, device=DEV), torch.zeros(f, f, dtype=torch.float64, device=DEV)


def _check(s, c, x, n_total=None):
    s_w, c_w = S.accumulate(x)
    s_b, c_b = S.accumulate_bound(x, n_total)
    s, c = s.cpu(), c.cpu()
    assert torch.isfinite(s).all() and torch.isfinite(c).all()
    assert torch.equal(c, c.t())                                    # exactly symmetric
    es, ec = ((s - s_w).abs() / s_b).max().item(), ((c - c_w).abs() / c_b).max().item()
    print(f"accumulate {tuple(x.shape)} {x.dtype}: worst error / bound: sum {es:.3f}, cov_sum {ec:.3f}")
    assert ((s - s_w).abs() <= s_b).all() and ((c - c_w).abs() <= c_b).all()


CASES = [(1, 16), (3, 16), (4, 64), (5, 64), (17, 192), (64, 768), (33, 2048), (7, 4096)]


@pytest.mark.parametrize("n,f", CASES)
def test_accumulate_f32(n, f):
    """|err| <= 8 N 2^-53 (|X|^T |X|) elementwise against the CPU's f64 X^T X, `sum` likewise; cov_sum exactly symmetric.  The buffer holds four more
    rows than N, filled with NaN: a read past row N shows as a non-finite state.  Observed on an MI355X: no element above 0.001 of the bound in one call (f32
    products are exact in f64 and the sums short), 0.015 of it over the five batches of test_accumulate_batches_one_after_another_and_rerun."""
    from dmvae_amd import ops
    x, xd = _x(n, f, torch.float32, rows=n + 4)
    s, c = _states(f)
    ops.fid_accumulate(xd, s, c)
    _check(s, c, x)


@pytest.mark.parametrize("n,f", [(5, 64), (17, 192)])
@pytest.mark.parametrize("dtype", [BF, torch.float64])
def test_accumulate_bf16_and_f64(n, f, dtype):
    from dmvae_amd import ops
    x, xd = _x(n, f, dtype, rows=n + 3)
    s, c = _states(f)
    ops.fid_accumulate(xd, s, c)
    _check(s, c, x)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_accumulate_with_a_leading_dimension_and_nan_around(dtype):
    """Row pitch 200 > F = 192, rows beyond N and columns beyond F filled with NaN: none of it is read."""
    from dmvae_amd import ops
    x, xd = _x(17, 192, dtype, rows=24, ld=200)
    assert xd.stride() == (200, 1) and not xd.is_contiguous()
    s, c = _states(192)
    ops.fid_accumulate(xd, s, c)
    _check(s, c, x)


def test_accumulate_batches_one_after_another_and_rerun():
    """Batches of 1, 3, 4, 17 and 8 rows into one state: within the bound of the whole (N = 33), and the same bits on a second run."""
    from dmvae_amd import ops
    x, xd = _x(33, 192, torch.float32)
    runs = []
    for _ in range(2):
        s, c = _states(192)
        for part in xd.split([1, 3, 4, 17, 8]):
            ops.fid_accumulate(part, s, c)
        runs.append((s.clone(), c.clone()))
    _check(*runs[0], x)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the state is read from the upper triangle, the owner rewrites the lower one: a one-shot pass over the same rows meets the same bound
    s, c = _states(192)
    ops.fid_accumulate(xd, s, c)
    _check(s, c, x)


def test_accumulate_refuses_what_it_does_not_cover():
    from dmvae_amd import _lib, ops
    s, c = _states(24)
    with pytest.raises(_lib.DmvaeHipError, match="multiple of 16"):
        ops.fid_accumulate(torch.zeros(4, 24, device=DEV), s, c)
    with pytest.raises(TypeError):
        ops.fid_accumulate(torch.zeros(4, 16, device=DEV, dtype=torch.float16), *_states(16))
    with pytest.raises(ValueError):
        ops.fid_accumulate(torch.zeros(4, 16, device=DEV), *_states(32))


# ---- resize ----------------------------------------------------------------------------------------------------------------------------------
def _images(h, w, dtype, seed=0):
    """B = 2, C = 3, uniform in [0, 1]; four rows of one channel exactly 0 and four rows of another exactly 1: the clamp and the boundary at 255."""
    g = torch.Generator().manual_seed(100 * h + w + seed)
    x = torch.rand(2, 3, h, w, generator=g)
    x[0, 0, 2:6] = 0.0
    x[1, 1, h - 6:h - 2] = 1.0
    return x.to(dtype)


@pytest.mark.parametrize("h,size", [(16, 19), (24, 29), (40, 13), (19, 19), (24, 299)])
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_resize_u8_against_the_formula(h, size, dtype):
    """Equal to the spec's uint8 at every stable pixel, at most one level off at the others, and at most 10 % of the pixels unstable.  With ATen's CPU
    f32 kernel in the kernel's place the same check gives no stable mismatch and unstable shares of 0.4 - 7.3 % (f32), 0.3 - 3.0 % (bf16) on these inputs."""
    from dmvae_amd import ops
    x = _images(h, h, dtype)
    S.check_resize(ops.fid_resize_u8(x.to(DEV), size), x, size)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_resize_u8_of_a_non_square_image(dtype):
    """H != W: each axis has its own scale; down along W, up along H."""
    from dmvae_amd import ops
    x = _images(12, 23, dtype)
    S.check_resize(ops.fid_resize_u8(x.to(DEV), 17), x, 17)


def test_resize_u8_clamps_what_lies_outside_0_1():
    from dmvae_amd import ops
    x = torch.tensor([-0.5, -1e-3, 0.0, 0.5, 1.0, 1.0 + 1e-3, 7.0]).view(1, 1, 1, 7).expand(1, 1, 7, 7).contiguous()
    got = ops.fid_resize_u8(x.to(DEV), 7).cpu()
    assert got[0, 0, 0].tolist() == [0, 0, 0, 127, 255, 255, 255]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
class StubExtractor(torch.nn.Module):
    """uint8 [B, 3, S, S] -> [B, 64]: average pool to 8 x 8, flatten, a fixed random [192, 64] projection."""

    def __init__(self):
        super().__init__()
        self.register_buffer("proj", torch.randn(192, 64, generator=torch.Generator().manual_seed(11)) / 192 ** 0.5)

    def forward(self, u8):
        return torch.nn.functional.adaptive_avg_pool2d(u8.float() / 255, 8).flatten(1) @ self.proj


def _stable_images(count, seed, lo=0.0, hi=1.0):
    """16-px images, uniform in [lo, hi], whose 19-px spec image has no unstable pixel, picked from seeded candidates by the spec alone: at such images the kernel's uint8
    output is the spec's (test_resize_u8_against_the_formula), so the extractor sees the same input on both sides and its f32 GEMM is the only non-f64 step."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.rand(2048, 3, 16, 16, generator=g) * (hi - lo) + lo
    _, stable = S.resize_u8(cand, 19)
    good = stable.flatten(1).all(1).nonzero().flatten()
    assert len(good) >= count, len(good)
    return cand[good[:count]]


def test_fid_end_to_end_with_a_stub_extractor():
    """FID(stub, eval_size=19) fed real and fake 16-px batches of 1, 5 and 2 images == the spec on the spec's uint8 images through the same stub on the CPU,
    within 1e-6 relative.  The images are picked so that the spec marks every pixel stable (`_stable_images`): the stub's f32 GEMM on the two devices is then the
    only step that is not f64.  Observed on an MI355X: 0.942093535634 against 0.942093630720, 1.0e-7 relative."""
    from dmvae_amd.fid import FID
    stub = StubExtractor()                                         # the CPU's copy: the same seeded projection
    real, fake = _stable_images(8, 1), _stable_images(8, 2, 0.1, 0.8)
    fid = FID(StubExtractor(), eval_size=19).to(DEV)
    for x, side in ((real, True), (fake, False)):
        for part in x.split([1, 5, 2]):
            fid.update(part.to(DEV), side)
    assert int(fid.real_features_num_samples) == 8 and int(fid.fake_features_num_samples) == 8
    got = fid.compute().item()
    want = S.fid_from_features(stub(S.resize_u8(real, 19)[0]), stub(S.resize_u8(fake, 19)[0]))
    print(f"FID end to end: {got:.12f}, spec {want:.12f}, relative difference {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-6 * want


class IdentityVAE(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def encode(self, x):
        return x

    def decode(self, z):
        return z


def test_fid_as_the_metric_of_evaluate():
    """evaluate(..., fid=obj) calls update(x01, False) and update(s01, True) per batch; with identity encode / decode both sides see the same images, so
    the states are equal bit for bit and the value is 0 up to the square roots of the covariance product's zero eigenvalues (8 samples, 64 features: at most 64
    of them, each computed as up to 64 * 2^-53 * |s|_2^2 <= 64 * 2^-53 * tr^2 in size; twice in the value, both signs).  Observed on an MI355X: -5.8e-8 on a
    trace of 1.42."""
    from dmvae_amd.evaluate import evaluate
    from dmvae_amd.fid import FID
    fid = FID(StubExtractor(), eval_size=19).to(DEV)
    calls = []
    inner = fid.update
    fid.update = lambda imgs, real: (calls.append((tuple(imgs.shape), bool(real))), inner(imgs, real))[1]
    imgs = _stable_images(8, 3)
    batches = [(b * 2 - 1, torch.zeros(len(b), dtype=torch.long)) for b in imgs.split([1, 5, 2])]
    out = evaluate(IdentityVAE().to(DEV), batches, num_samples=8, device=DEV, fid=fid)
    assert calls == [((n, 3, 16, 16), r) for n in (1, 5, 2) for r in (False, True)]
    assert int(fid.real_features_num_samples) == 8 and int(fid.fake_features_num_samples) == 8
    assert torch.equal(fid.real_features_cov_sum, fid.fake_features_cov_sum) and torch.equal(fid.real_features_sum, fid.fake_features_sum)
    tr = 2 * fid.statistics(True)[1].trace().item()
    print(f"evaluate: FID {out['FID']:.3e} on identical sides, trace {tr:.4f}")
    assert out["images"] == 8 and out["FID"] is not None and abs(out["FID"]) <= 1e-9 * tr + 4 * 64 * (64 * 2.0 ** -53) ** 0.5 * tr
