"""The all-pairs metrics of the evaluation tail on the MI355X (-m gpu): csrc/manifold.hip's radii, memberships and KID subset values against the numpy
restatement of tests/manifold_spec.py -- within the bounds derived there on Gaussian data, bit for bit on small-integer data (where every product and sum is
exact in f64), with their rerun / permutation / slot identities -- and dmvae_amd.fidelity's `FeatureBank` / `compute(kid=True, prc=True)` around a stub
extractor.  The comparison side is numpy on the host; no test opts into stock PyTorch.

Inputs are views (row pitch F + 8, four more rows, NaN outside) and outputs sit inside sentinel buffers: a read past a row's features or past the last row
shows as a NaN, a write outside the result as a changed sentinel."""
import numpy as np
import pytest
import torch

import manifold_spec as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
PAD = 64


def _gauss(n, f, dtype, seed=0):
    """-> x [n, f] of `dtype` on the CPU: unit Gaussian rows."""
    return torch.randn(n, f, generator=torch.Generator().manual_seed(1000 * n + f + seed), dtype=torch.float64).to(dtype)


def _ints(n, f, lo, hi, seed=0):
    return torch.randint(lo, hi + 1, (n, f), generator=torch.Generator().manual_seed(77 * n + f + seed)).to(F32)


def _view(x):
    """The same values on the device as a view with row pitch F + 8 of a buffer with four more rows, NaN everywhere outside the view."""
    n, f = x.shape
    buf = torch.full((n + 4, f + 8), float("nan"), dtype=x.dtype)
    buf[:n, :f] = x
    v = buf.to(DEV)[:n, :f]
    assert v.stride() == (f + 8, 1)
    return v


def _sentinel(n, dtype):
    value = 250 if dtype == torch.uint8 else -7.25
    big = torch.full((n + 2 * PAD,), value, dtype=dtype, device=DEV)
    return big, big[PAD:PAD + n], value


def _untouched(big, n, value):
    return bool((big[:PAD] == value).all() and (big[PAD + n:] == value).all())


def _radii(x, k):
    """ops.knn_radius into a sentinel buffer, twice: -> f64 numpy [n]."""
    from dmvae_amd import ops
    xd, n = _view(x), x.shape[0]
    runs = []
    for _ in range(2):
        big, out, value = _sentinel(n, F64)
        got = ops.knn_radius(xd, k, out=out)
        assert got.data_ptr() == out.data_ptr() and _untouched(big, n, value)
        runs.append(got.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])                           # a rerun gives the same bits
    return runs[0]


def _members(q, r, radius2):
    from dmvae_amd import ops
    qd, rd, nq = _view(q), _view(r), q.shape[0]
    rad = torch.from_numpy(np.asarray(radius2, dtype=np.float64)).to(DEV)
    runs = []
    for _ in range(2):
        big, out, value = _sentinel(nq, torch.uint8)
        got = ops.manifold_member(qd, rd, rad, out=out)
        assert got.data_ptr() == out.data_ptr() and _untouched(big, nq, value)
        runs.append(got.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]) and runs[0].dtype == np.uint8 and set(runs[0].tolist()) <= {0, 1}
    return runs[0]


def _mmd2(x, y, t1, t2, *args):
    from dmvae_amd import ops
    xd, yd, s = _view(x), _view(y), len(t1)
    i1, i2 = torch.from_numpy(t1).to(DEV), torch.from_numpy(t2).to(DEV)
    runs = []
    for _ in range(2):
        big, out, value = _sentinel(s, F64)
        got = ops.kid_mmd2(xd, yd, i1, i2, *args, out=out)
        assert got.data_ptr() == out.data_ptr() and _untouched(big, s, value)
        runs.append(got.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
    return runs[0]


# ---- radii -------------------------------------------------------------------------------------------------------------------------------------------
# one tile and its edges (9, 15, 16, 17), the 64-row block and its edges (63, 64, 65), several blocks (130), 2049 rows: 33 row blocks x 16 column splits of 33
# column tiles; F = 48 is three K-chunks, 2048 is 128
KNN_SHAPES = [(9, 16, 1), (9, 48, 8), (15, 16, 3), (16, 48, 1), (17, 16, 8), (63, 48, 3), (64, 16, 8), (65, 48, 1), (130, 16, 3), (130, 48, 8), (17, 2048, 3),
              (65, 2048, 8), (2049, 16, 3)]


@pytest.mark.parametrize("n,f,k", KNN_SHAPES)
@pytest.mark.parametrize("dtype", [F32, F64])
def test_knn_radius_against_the_spec(n, f, k, dtype):
    """|radius2 - spec| <= radius_bound per row (the bound of any summation order, tests/manifold_spec.py) on unit Gaussian rows.
    Observed on an MI355X: worst error / bound 0.042 over the shapes and both dtypes (bounds 3e-13 ... 4e-9, the largest at F = 2048 where d2 ~ 4000)."""
    x = _gauss(n, f, dtype)
    got = _radii(x, k)
    want, bound = M.knn_radius(x.double().numpy(), k), M.radius_bound(x.double().numpy())
    assert got.shape == (n,) and got.dtype == np.float64 and np.isfinite(got).all()
    ratio = (np.abs(got - want) / bound).max()
    print(f"knn_radius {(n, f, k)} {dtype}: worst error / bound {ratio:.4f} (bound {bound.max():.2e})")
    assert ratio <= 1.0


# ---- membership -----------------------------------------------------------------------------------------------------------------------------------------
MEMBER_SHAPES = [(1, 9, 16, 1), (9, 15, 48, 3), (15, 9, 16, 8), (16, 17, 48, 1), (17, 16, 16, 3), (63, 65, 48, 3), (64, 64, 16, 1), (65, 63, 2048, 3),
                 (130, 130, 48, 8), (1, 130, 16, 3), (130, 17, 16, 3), (2049, 130, 16, 3), (130, 2049, 16, 3)]


def _member_case(nq, nr, f, dtype):
    """Queries: half fresh Gaussian rows (outside most balls at these sizes), half reference rows moved by a small Gaussian step (inside)."""
    r = _gauss(nr, f, dtype, seed=1)
    q = _gauss(nq, f, dtype, seed=2)
    step = _gauss(nq, f, torch.float64, seed=3) * 0.05
    near = (r[torch.arange(nq) % nr].double() + step).to(dtype)
    q[1::2] = near[1::2]
    return q, r


@pytest.mark.parametrize("nq,nr,f,k", MEMBER_SHAPES)
@pytest.mark.parametrize("dtype", [F32, F64])
def test_manifold_member_against_the_spec(nq, nr, f, k, dtype):
    """The radii are the kernel's own.  A query is undecided when the spec, with the distance and radius bounds, cannot tell on which side of every deciding
    ball it lies; the cap on undecided queries is zero (the seeds are checked on the CPU: margins ~1e-3 against bounds ~1e-12), every query must match."""
    q, r = _member_case(nq, nr, f, dtype)
    rad = _radii(r, k)
    qn, rn = q.double().numpy(), r.double().numpy()
    want_rad, err = M.knn_radius(rn, k), M.radius_bound(rn)
    assert (np.abs(rad - want_rad) <= err).all()
    assert not M.member_undecided(qn, rn, want_rad, err).any()
    got, want = _members(q, r, rad), M.manifold_member(qn, rn, want_rad)
    print(f"manifold_member {(nq, nr, f, k)} {dtype}: {int(want.sum())} of {nq} inside")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("nq,f", [(1, 16), (17, 48), (65, 2048)])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_manifold_member_against_one_reference_row(nq, f, dtype):
    """Nr = 1 (every staged reference row is row 0 again) with a radius given by hand: the median of the queries' exact distances, moved off every one of
    them, so that some are inside and, from two queries on, some outside; the radius is exact, the distances' bound alone decides."""
    q, r = _member_case(nq, 1, f, dtype)
    qn, rn = q.double().numpy(), r.double().numpy()
    d = np.sort(M.dist2(qn, rn)[:, 0])
    rad = np.array([d[0] + 1.0 if nq == 1 else 0.5 * (d[nq // 2 - 1] + d[nq // 2])])
    assert not M.member_undecided(qn, rn, rad, np.zeros(1)).any()
    want = M.manifold_member(qn, rn, rad)
    assert want.sum() == max(nq // 2, 1)
    assert np.array_equal(_members(q, r, rad), want)
    assert _members(q, r, np.array([d[0] * 0.5])).sum() == 0


# ---- exact data: bit for bit ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,f,k", [(17, 16, 1), (65, 48, 3), (25, 2048, 8), (130, 16, 3)])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_integer_features_give_the_specs_bits(n, f, k, dtype):
    """Features in {-3 .. 3}: every product and sum is an integer far below 2^53.  Radii, memberships (queries also integer) and, with gamma = 2^-4,
    coef0 = 1 and degree 3, the subset values equal the spec bit for bit.  Rows 0 .. 4 are repeated k more times: their (k + 1)-th value is exactly 0."""
    x = _ints(n, f, -3, 3)
    x = torch.cat([x] + [x[:5]] * k).to(dtype)
    got = _radii(x, k)
    want = M.knn_radius(x.double().numpy(), k)
    assert np.array_equal(got, want) and (got[:5] == 0.0).all() and (got[n:] == 0.0).all() and (got[5:n] > 0).any()
    q = torch.cat([_ints(n, f, -3, 3, seed=5), x[:7]]).to(dtype)
    assert np.array_equal(_members(q, x, got), M.manifold_member(q.double().numpy(), x.double().numpy(), want))
    y = _ints(n + 3, f, -3, 3, seed=9).to(dtype)
    t1, t2 = M.kid_subset_tables(len(x), len(y), 3, min(n, 65), 4)
    args = (3, 2.0 ** -4, 1.0)
    assert np.array_equal(_mmd2(x, y, t1, t2, *args), M.kid_mmd2(x.double().numpy(), y.double().numpy(), t1, t2, *args))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_points_on_a_line_and_a_query_on_a_balls_surface(dtype):
    """r_j = 10 j e_0, j < 70 (two row blocks): every radius2 with k = 1 is exactly 100, with k = 3 it is 400 inside and 900 at the two ends.  Queries:
    r_0 + 10 e_1 lies exactly ON r_0's ball (and 200 from r_1): `<=` counts it inside; one more unit along e_2 and it is outside every ball; 25 e_0 is
    inside two balls; a query 10 e_1 off the LAST reference row (row 69, the second block's ragged end) is on its surface."""
    n = 70
    r = torch.zeros(n, 16, dtype=dtype)
    r[:, 0] = 10.0 * torch.arange(n)
    rad = _radii(r, 1)
    assert np.array_equal(rad, np.full(n, 100.0))
    steps = np.minimum(np.minimum(np.arange(n), n - 1 - np.arange(n)), 1)
    assert np.array_equal(_radii(r, 3), np.where(steps == 0, 900.0, 400.0))
    q = torch.zeros(5, 16, dtype=dtype)
    q[0, 1] = 10.0
    q[1, 1], q[1, 2] = 10.0, 1.0
    q[2, 0] = 25.0
    q[3, 0], q[3, 1] = 690.0, 10.0
    q[4, 0], q[4, 1], q[4, 2] = 690.0, 10.0, 1.0
    assert _members(q, r, rad).tolist() == [1, 0, 1, 1, 0] == M.manifold_member(q.double().numpy(), r.double().numpy(), rad).tolist()


# ---- KID ---------------------------------------------------------------------------------------------------------------------------------------------------
KID_SHAPES = [(9, 15, 9, 3, 16), (17, 16, 16, 2, 48), (65, 63, 17, 4, 16), (130, 130, 65, 3, 48), (65, 65, 64, 2, 2048), (130, 140, 130, 2, 16), (9, 9, 2, 5, 16)]


@pytest.mark.parametrize("n1,n2,m,s,f", KID_SHAPES)
@pytest.mark.parametrize("dtype", [F32, F64])
def test_kid_mmd2_against_the_spec(n1, n2, m, s, f, dtype):
    """|mmd2 - spec| <= kid_bound per subset at the library's defaults (degree 3, gamma 1 / F, coef0 1), at degree 1 and at degree 8.
    Observed on an MI355X: worst error / bound 0.012 (at m = 2, where the bound is 7.6e-14); 0.003 at m = 9, at most 0.002 from m = 16 on (bounds 1e-14 ... 1e-9)."""
    x, y = _gauss(n1, f, dtype, seed=4), _gauss(n2, f, dtype, seed=5) + 0.25
    t1, t2 = M.kid_subset_tables(n1, n2, s, m, 6)
    for args in ((3, None, 1.0), (1, 0.5, 0.0), (8, 1.0 / f, 0.5)):
        got = _mmd2(x, y, t1, t2, *args)
        want, bound = (fn(x.double().numpy(), y.double().numpy(), t1, t2, *args) for fn in (M.kid_mmd2, M.kid_bound))
        assert got.shape == (s,) and got.dtype == np.float64 and np.isfinite(got).all()
        ratio = (np.abs(got - want) / bound).max()
        print(f"kid_mmd2 {(n1, n2, m, s, f)} {dtype} degree {args[0]}: worst error / bound {ratio:.4f} (bound {bound.max():.2e}, |mmd2| {np.abs(want).max():.2e})")
        assert ratio <= 1.0


# ---- identities, bit for bit ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,f", [(130, 48), (2049, 16)])
def test_permutation_and_slot_identities(n, f):
    """Permuting the reference rows permutes radius2 and leaves the memberships unchanged; permuting the queries permutes the output; a subset's value does not
    depend on its slot in the table, nor on the subsets around it."""
    r, q = _gauss(n, f, F32, seed=1), _member_case(67, n, f, F32)[0]
    perm, qperm = np.random.RandomState(n).permutation(n), np.random.RandomState(f).permutation(67)
    rad = _radii(r, 3)
    rad_p = _radii(r[perm], 3)
    assert np.array_equal(rad_p, rad[perm])
    mem = _members(q, r, rad)
    assert 0 < mem.sum() < 67
    assert np.array_equal(_members(q, r[perm], rad_p), mem)
    assert np.array_equal(_members(q[qperm], r, rad), mem[qperm])
    y = _gauss(n, f, F32, seed=8)
    t1, t2 = M.kid_subset_tables(n, n, 5, 65, 1)
    base = _mmd2(r, y, t1, t2)
    order = np.array([3, 0, 4, 2, 1])
    assert np.array_equal(_mmd2(r, y, t1[order], t2[order]), base[order])
    assert np.array_equal(_mmd2(r, y, t1[2:3], t2[2:3]), base[2:3])
    assert len(set(base.tolist())) == 5


def test_ops_refuse_what_they_do_not_cover():
    from dmvae_amd import _lib, ops
    x = _gauss(20, 16, F32).to(DEV)
    rad = torch.zeros(20, dtype=F64, device=DEV)
    idx = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(TypeError):
        ops.knn_radius(x.half(), 3)
    with pytest.raises(TypeError):
        ops.knn_radius(x.bfloat16(), 3)
    with pytest.raises(TypeError):
        ops.manifold_member(x, x.double(), rad)
    with pytest.raises(TypeError):
        ops.manifold_member(x, x, rad.float())
    with pytest.raises(TypeError):
        ops.kid_mmd2(x, x, idx.int(), idx)
    with pytest.raises(_lib.DmvaeHipError):
        ops.knn_radius(x.cpu(), 3)
    for k in (0, 9):
        with pytest.raises(ValueError, match="k"):
            ops.knn_radius(x, k)
    with pytest.raises(ValueError):
        ops.knn_radius(x[:3], 3)                                      # N <= k
    with pytest.raises(ValueError):
        ops.knn_radius(torch.zeros(20, 24, device=DEV), 3)            # F % 16
    with pytest.raises(ValueError):
        ops.manifold_member(x, x, rad[:19])
    with pytest.raises(ValueError, match="degree"):
        ops.kid_mmd2(x, x, idx, idx, degree=9)
    with pytest.raises(ValueError, match="m >= 2"):
        ops.kid_mmd2(x, x, idx[:, :1].contiguous(), idx[:, :1].contiguous())
    lib, calls = _lib.lib(), []
    real = lib.dmvae_kid_mmd2
    lib.dmvae_kid_mmd2 = lambda *a: calls.append(a) or real(*a)
    try:
        for bad in (20, -1):                                          # a table entry out of range: refused before any launch
            t = idx.clone()
            t[1, 2] = bad
            with pytest.raises(ValueError, match="idx"):
                ops.kid_mmd2(x, x, t, idx)
            with pytest.raises(ValueError, match="idx"):
                ops.kid_mmd2(x, x, idx, t)
    finally:
        lib.dmvae_kid_mmd2 = real
    assert calls == []


# ---- FeatureBank / FidelityMetrics -------------------------------------------------------------------------------------------------------------------------
class StubExtractor(torch.nn.Module):
    """f32 [B, 3, S, S] -> (features [B, 16], logits [B, 8]): average pool to 4 x 4, flatten, two fixed random matrices."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.register_buffer("wf", torch.randn(48, 16, generator=g) / 48 ** 0.5)
        self.register_buffer("wl", torch.randn(48, 8, generator=g) * 0.5)

    def forward(self, x):
        v = torch.nn.functional.adaptive_avg_pool2d(x, 4).flatten(1)
        return v @ self.wf, v @ self.wl


def _u8(b, c, h, w, seed=0):
    return torch.randint(0, 256, (b, c, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(1000 * h + w + seed))


def _metrics(**kw):
    from dmvae_amd.fidelity import FidelityMetrics
    return FidelityMetrics(StubExtractor(), num_features=16, num_classes=8, eval_size=32, **kw).to(DEV)


def test_fidelity_metrics_kid_and_prc_end_to_end_with_a_stub_extractor(tmp_path):
    """40 sampled and 48 real uint8 images of 24 x 20 through resize kernel -> stub -> the banks (the real side leaves the fake side's states alone).
    compute(kid=True, prc=True, kid_subsets=4, kid_subset_size=16) against the spec on the banks' own features: precision / recall / f_score exactly (no query
    is undecided), the KID mean / std within the derived bound.  Batch splits of 1 + 7 + 32 and the rows in reverse with their indices give the same bits;
    a reference bank saved and loaded gives the same result; without the flags the result is that of an object that keeps nothing.
    Observed on an MI355X: KID worst error / bound 0.002 (bound 2.3e-13, mean -8.486e-4); precision 0.9000, recall 0.9375, f_score 0.9184."""
    fake, real = _u8(40, 3, 24, 20).permute(0, 2, 3, 1).contiguous(), _u8(48, 3, 24, 20, seed=7).permute(0, 2, 3, 1).contiguous()
    m, plain, parts, rev = _metrics(keep_features=True), _metrics(), _metrics(keep_features=True), _metrics(keep_features=True)
    for part in fake.split(8):
        m.update_uint8(part.to(DEV))
        plain.update_uint8(part.to(DEV))
    state = (m.num_samples, m.features_sum.clone(), m.features_cov_sum.clone(), len(m.isc))
    for part in real.split(16):
        m.update_reference_uint8(part.to(DEV))
    assert state[0] == m.num_samples and torch.equal(state[1], m.features_sum) and torch.equal(state[2], m.features_cov_sum) and state[3] == len(m.isc)
    assert len(m.bank) == 40 and len(m.reference_bank) == 48 and plain.bank is None and m.bank.features.is_cuda
    assert m.compute(splits=5, rng_seed=3) == plain.compute(splits=5, rng_seed=3)
    kw = dict(splits=5, rng_seed=3, kid=True, prc=True, kid_subsets=4, kid_subset_size=16)
    out = m.compute(**kw)
    assert list(out) == ["inception_score_mean", "inception_score_std", "kernel_inception_distance_mean", "kernel_inception_distance_std", "precision",
                         "recall", "f_score"]
    x, y = m.bank.features.cpu().numpy(), m.reference_bank.features.cpu().numpy()
    t1, t2 = M.kid_subset_tables(40, 48, 4, 16, 3)
    want, kb = M.kid_mmd2(x, y, t1, t2), M.kid_bound(x, y, t1, t2)
    got = m.kid_values(4, 16, rng_seed=3).cpu().numpy()
    print(f"FidelityMetrics KID: worst error / bound {(np.abs(got - want) / kb).max():.4f} (bound {kb.max():.2e}); mean {np.mean(want):.6e}")
    assert (np.abs(got - want) <= kb).all()
    assert out["kernel_inception_distance_mean"] == float(np.mean(got)) and out["kernel_inception_distance_std"] == float(np.std(got))
    for q, r in ((x, y), (y, x)):
        assert not M.member_undecided(q, r, M.knn_radius(r, 3), M.radius_bound(r)).any()
    p, r, fs = M.precision_recall(x, y, 3)
    print(f"FidelityMetrics precision {p:.4f} recall {r:.4f} f_score {fs:.4f}")
    assert (out["precision"], out["recall"], out["f_score"]) == (p, r, fs) and 0 < p < 1 and 0 < r < 1
    # the same features in other batch splits (the buffer grows from 64 rows), and the rows in reverse with their indices: the same bits.  The splits are
    # made behind the extractor: the stub's matrix product is not this package's and may depend on its batch
    feats, logits, ref = m.bank.features.clone(), m.isc.logits.clone(), m.reference_bank.features.clone()
    for fp, lp in zip(feats.split([1, 7, 32]), logits.split([1, 7, 32])):
        parts.update_features(fp, lp)
    for part in ref.split([5, 43]):
        parts.update_reference_features(part)
    rev.update_features(feats.flip(0), logits.flip(0), torch.arange(40).flip(0))
    rev.update_reference_features(ref.flip(0), torch.arange(48).flip(0))
    assert torch.equal(parts.bank.features, feats) and torch.equal(rev.bank.features, feats.flip(0)) and rev.bank.index.tolist() == list(range(39, -1, -1))
    assert parts.compute(**kw) == out
    got_rev = rev.compute(**kw)
    assert all(got_rev[key] == out[key] for key in out if not key.startswith("inception_score"))
    # the real side from a file
    m.reference_bank.save(tmp_path / "real.npz")
    loaded = _metrics(keep_features=True)
    loaded.load_reference_features(tmp_path / "real.npz")
    assert loaded.reference_bank.features.is_cuda
    loaded.update_features(feats, logits)
    assert loaded.compute(**kw) == out
    # .to(...) moves the banks with the buffers
    loaded.to("cpu")
    assert not loaded.bank.features.is_cuda and not loaded.reference_bank.features.is_cuda and torch.equal(loaded.bank.features, feats.cpu())
    loaded.to(DEV)
    assert loaded.bank.features.is_cuda and loaded.reference_bank.is_global and loaded.compute(**kw) == out
    with pytest.raises(RuntimeError, match="keep_features"):
        plain.compute(prc=True)
    with pytest.raises(RuntimeError, match="real-side"):
        _metrics(keep_features=True).compute(kid=True)
