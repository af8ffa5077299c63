"""CPU: tests/manifold_spec.py against closed forms (points on a line, identical sets, a hand-worked MMD^2), `kid_subset_tables` against direct RandomState
calls, dmvae_amd.fidelity's stock f64 route (behind DMVAE_ALLOW_STOCK=1) against the spec, `FeatureBank`'s growth and file format, the missing-bank errors,
and `compute()` without the new flags against what it returned before they existed.  The kernels are covered by tests/test_gpu_manifold.py."""
import os
import socket
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import manifold_spec as M
from dmvae_amd import _lib
from dmvae_amd import fidelity as Fd
from dmvae_amd.fidelity import FeatureBank, kid_subset_tables      # noqa: F401  (the spec alone is no test of this package: without these nothing here runs)


def _gauss(n, f, seed, scale=1.0):
    return (torch.randn(n, f, generator=torch.Generator().manual_seed(1000 * n + f + seed), dtype=torch.float64) * scale).float()


# ---- the spec against closed forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 8])
def test_spec_radii_of_equally_spaced_points_on_a_line(k):
    """x_i = 3 i e_0, i < 20: the k-th neighbour of an interior point is ceil(k / 2) steps away, of an end point k steps -- radius2 = 9 steps^2, exactly."""
    n = 20
    x = np.zeros((n, 16))
    x[:, 0] = 3.0 * np.arange(n)
    steps = np.array([sorted(abs(i - j) for j in range(n))[k] for i in range(n)], dtype=np.float64)
    assert steps[0] == k and steps[n // 2] == (k + 1) // 2
    assert np.array_equal(M.knn_radius(x, k), 9.0 * steps * steps)
    perm = np.random.RandomState(k).permutation(n)
    assert np.array_equal(M.knn_radius(x[perm], k), (9.0 * steps * steps)[perm])


def test_spec_identical_sets_have_precision_and_recall_one_and_duplicates_radius_zero():
    x = _gauss(40, 16, 1).numpy()
    assert M.precision_recall(x, x, 3) == (1.0, 1.0, 1.0)
    far = x + 100.0
    assert M.precision_recall(x, far, 3) == (0.0, 0.0, 0.0)
    dup = np.concatenate([x[:5]] * 4 + [x[5:]])                       # rows 0..4 four times each: three other rows at distance 0
    r = M.knn_radius(dup, 3)
    assert (r[:20] == 0.0).all() and (r[20:] > 0.0).all()
    # `<=`: a query on the surface of a ball is inside
    line = np.zeros((6, 16))
    line[:, 0] = 10.0 * np.arange(6)
    rad = M.knn_radius(line, 1)
    assert np.array_equal(rad, np.full(6, 100.0))
    q = np.zeros((3, 16))
    q[0, 1], q[1, 1], q[1, 2], q[2, 0] = 10.0, 10.0, 1.0, 25.0        # on r_0's surface; just outside it; between r_2 and r_3, inside both
    assert M.manifold_member(q, line, rad).tolist() == [1, 0, 1]
    assert M.member_undecided(q, line, rad, np.zeros(6)).tolist() == [True, False, False]      # the exact tie is the one thing a bound cannot decide


def test_spec_mmd2_of_small_integer_sets_worked_by_hand():
    """F = 16 with two used coordinates, gamma = 1, coef0 = 1, degree 2, m = 2: x = {(1, 0), (0, 1)}, y = {(1, 1), (2, 0)}.
    K_xx off-diagonal: (0 + 1)^2 twice = 2.  K_yy off-diagonal: (2 + 1)^2 twice = 18.  K_xy: (1 + 1)^2, (2 + 1)^2, (1 + 1)^2, (0 + 1)^2 = 4 + 9 + 4 + 1 = 18.
    mmd2 = (2 + 18) / 2 - 2 * 18 / 4 = 1."""
    x, y = np.zeros((2, 16)), np.zeros((2, 16))
    x[0, 0], x[1, 1] = 1, 1
    y[0, 0], y[0, 1], y[1, 0] = 1, 1, 2
    idx = np.array([[0, 1]])
    assert M.kid_mmd2(x, y, idx, idx, degree=2, gamma=1.0, coef0=1.0).tolist() == [1.0]
    assert M.kid_mmd2(x, y, idx[:, ::-1], idx, degree=2, gamma=1.0, coef0=1.0).tolist() == [1.0]
    assert M.kid_mmd2(x, x, idx, idx, degree=2, gamma=1.0, coef0=1.0).tolist() == [(1 + 1) - 2 * (4 + 1 + 1 + 4) / 4]      # the biased cross term stays
    # degree 1, coef0 0: the kernel is the dot product; mmd2 = (0 + 4) / 2 - 2 (1 + 2 + 1 + 0) / 4 = 0
    assert M.kid_mmd2(x, y, idx, idx, degree=1, gamma=1.0, coef0=0.0).tolist() == [0.0]
    assert (M.kid_bound(x, y, idx, idx, 2, 1.0, 1.0) < 1e-12).all() and (M.kid_bound(x, y, idx, idx, 2, 1.0, 1.0) > 0).all()


def test_the_bounds_cover_a_second_evaluation_in_another_order():
    """The derived bounds against an evaluation that differs from the spec's by its order: reversed features (and longdouble accumulation for the distance)."""
    x, y = _gauss(65, 48, 2).numpy().astype(np.float64), _gauss(63, 48, 3).numpy().astype(np.float64)
    other = M.dist2(x[:, ::-1].copy(), y[:, ::-1].copy())
    e = M.dist2_bound(x, y)
    assert (np.abs(other - M.dist2(x, y)) <= e).all() and e.max() < 1e-11
    xl, yl = x.astype(np.longdouble), y.astype(np.longdouble)
    exact = ((xl[:, None, :] - yl[None, :, :]) ** 2).sum(axis=2)
    assert (np.abs(M.dist2(x, y) - exact.astype(np.float64)) <= e).all()
    t1, t2 = M.kid_subset_tables(65, 63, 3, 17, 1)
    a, b = M.kid_mmd2(x, y, t1, t2), M.kid_mmd2(x[:, ::-1].copy(), y[:, ::-1].copy(), t1, t2)
    assert (np.abs(a - b) <= M.kid_bound(x, y, t1, t2)).all() and M.kid_bound(x, y, t1, t2).max() < 1e-12


# ---- kid_subset_tables ------------------------------------------------------------------------------------------------------------------------------
def test_kid_subset_tables_are_the_librarys_draws():
    for n1, n2, s, m, seed in ((40, 30, 4, 16, 0), (1000, 1200, 100, 1000, 0), (17, 17, 3, 17, 5)):
        t1, t2 = Fd.kid_subset_tables(n1, n2, s, m, seed)
        rng = np.random.RandomState(seed)
        for k in range(s):
            assert np.array_equal(t1[k], rng.choice(n1, m, replace=False)) and np.array_equal(t2[k], rng.choice(n2, m, replace=False))
        assert t1.dtype == np.int64 and t1.shape == t2.shape == (s, m)
        assert all(len(set(row)) == m for row in t1.tolist()) and t1.max() < n1 and t2.max() < n2
        w1, w2 = M.kid_subset_tables(n1, n2, s, m, seed)
        assert np.array_equal(t1, w1) and np.array_equal(t2, w2)
    assert not np.array_equal(Fd.kid_subset_tables(40, 30, 4, 16, 0)[0], Fd.kid_subset_tables(40, 30, 4, 16, 1)[0])
    with pytest.raises(ValueError):
        Fd.kid_subset_tables(40, 15, 4, 16)
    with pytest.raises(ValueError):
        Fd.kid_subset_tables(40, 30, 0, 16)
    with pytest.raises(ValueError):
        Fd.kid_subset_tables(40, 30, 4, 1)


# ---- the stock route against the spec -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,f,k", [(9, 15, 16, 1), (65, 63, 48, 3), (130, 64, 16, 8)])
def test_stock_route_against_the_spec(n, m, f, k):
    x, y = _gauss(n, f, 0), _gauss(m, f, 1)
    rad, bound = M.knn_radius(y.numpy(), k), M.radius_bound(y.numpy())
    got = Fd._stock_knn_radius(y, k).numpy()
    assert got.dtype == np.float64 and (np.abs(got - rad) <= bound).all() and bound.max() < 1e-11
    und = M.member_undecided(x.numpy(), y.numpy(), rad, bound)
    assert not und.any()
    assert np.array_equal(Fd._stock_manifold_member(x, y, torch.from_numpy(got)).numpy(), M.manifold_member(x.numpy(), y.numpy(), rad))
    t1, t2 = M.kid_subset_tables(n, m, 3, min(n, m, 17), 2)
    for degree, gamma, coef0 in ((3, None, 1.0), (1, 0.25, 0.0), (8, 1 / 64, 0.5)):
        want, kb = M.kid_mmd2(x.numpy(), y.numpy(), t1, t2, degree, gamma, coef0), M.kid_bound(x.numpy(), y.numpy(), t1, t2, degree, gamma, coef0)
        got = Fd._stock_kid_mmd2(x, y, torch.from_numpy(t1), torch.from_numpy(t2), degree, gamma, coef0).numpy()
        assert (np.abs(got - want) <= kb).all(), (np.abs(got - want) / kb).max()


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
    return Fd.FidelityMetrics(StubExtractor(), num_features=16, num_classes=8, eval_size=32, **kw)


def test_fidelity_metrics_kid_and_prc_on_the_stock_route(monkeypatch):
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    fake, real = _u8(40, 3, 24, 20).permute(0, 2, 3, 1).contiguous(), _u8(48, 3, 24, 20, seed=7).permute(0, 2, 3, 1).contiguous()
    m, plain = _metrics(keep_features=True), _metrics()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for part in fake.split(8):
            m.update_uint8(part)
            plain.update_uint8(part)
        before = (m.num_samples, m.features_sum.clone(), m.features_cov_sum.clone(), len(m.isc))
        for part in real.split(16):
            m.update_reference_uint8(part)
    assert before[0] == m.num_samples == 40 and torch.equal(before[1], m.features_sum) and torch.equal(before[2], m.features_cov_sum) and len(m.isc) == before[3]
    assert len(m.bank) == 40 and len(m.reference_bank) == 48 and plain.bank is None and plain.reference_bank is None
    assert m.compute(splits=5, rng_seed=3) == plain.compute(splits=5, rng_seed=3)                      # the flags off: the same keys and values
    out = m.compute(splits=5, rng_seed=3, kid=True, prc=True, kid_subsets=4, kid_subset_size=16)
    assert sorted(out) == ["f_score", "inception_score_mean", "inception_score_std", "kernel_inception_distance_mean", "kernel_inception_distance_std",
                           "precision", "recall"]
    x, y = m.bank.features.numpy(), m.reference_bank.features.numpy()
    t1, t2 = M.kid_subset_tables(40, 48, 4, 16, 3)
    want, kb = M.kid_mmd2(x, y, t1, t2), M.kid_bound(x, y, t1, t2)
    assert abs(out["kernel_inception_distance_mean"] - np.mean(want)) <= kb.max()
    assert abs(out["kernel_inception_distance_std"] - np.std(want)) <= 2 * kb.max()
    for q, r in ((x, y), (y, x)):
        assert not M.member_undecided(q, r, M.knn_radius(r, 3), M.radius_bound(r)).any()
    p, r, fs = M.precision_recall(x, y, 3)
    assert (out["precision"], out["recall"], out["f_score"]) == (p, r, fs)
    # image indices given in reverse arrival order: the subsets follow the indices, not the arrival
    rev = _metrics(keep_features=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rev.update_uint8(fake.flip(0), torch.arange(40).flip(0))
        rev.update_reference_uint8(real.flip(0), torch.arange(48).flip(0))
    got = rev.compute(splits=5, rng_seed=3, kid=True, prc=True, kid_subsets=4, kid_subset_size=16)
    assert abs(got["kernel_inception_distance_mean"] - out["kernel_inception_distance_mean"]) <= 2 * kb.max()
    assert (got["precision"], got["recall"]) == (out["precision"], out["recall"])


def test_feature_bank_grows_saves_and_loads(monkeypatch, tmp_path):
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    x, index = _gauss(257, 16, 4), torch.arange(257) * 3 + 5
    bank = Fd.FeatureBank(16)
    assert len(bank) == 0 and bank.features.shape == (0, 16) and bank.index.shape == (0,)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for part, idx in zip(x.split([1, 3, 17, 236]), index.split([1, 3, 17, 236])):      # 64 rows of capacity grow to 257
            bank.update(part, idx)
    assert len(bank) == 257 and torch.equal(bank.features, x) and torch.equal(bank.index, index) and bank.features.dtype == torch.float32
    feats, order = bank.ordered()
    assert torch.equal(feats, x) and np.array_equal(order, np.arange(257))
    bank.save(tmp_path / "bank.npz")
    with np.load(tmp_path / "bank.npz") as z:
        assert sorted(z.files) == ["features", "index"] and z["features"].dtype == np.float32 and z["index"].dtype == np.int64
        assert np.array_equal(z["features"], x.numpy()) and np.array_equal(z["index"], index.numpy())
    other = Fd.FeatureBank(16)
    other.update(x[:3])
    assert other.index.tolist() == [0, 1, 2]                           # default indices: arrival order
    other.load(tmp_path / "bank.npz")
    assert len(other) == 257 and torch.equal(other.features, x) and torch.equal(other.index, index)
    m = _metrics(keep_features=True)
    m.load_reference_features(tmp_path / "bank.npz")
    assert torch.equal(m.reference_bank.features, x) and torch.equal(m.reference_bank.index, index)
    with pytest.raises(ValueError):
        Fd.FeatureBank(32).load(tmp_path / "bank.npz")
    with pytest.raises(ValueError):
        bank.update(torch.zeros(2, 17))
    with pytest.raises(ValueError):
        bank.update(torch.zeros(2, 16), torch.arange(3))
    with pytest.raises(ValueError):
        Fd.FeatureBank(24)
    bank.reset()
    assert len(bank) == 0
    m.reset()
    assert len(m.bank) == 0 and len(m.reference_bank) == 257           # the real side stays, as loaded statistics do


def test_feature_bank_refuses_cpu_tensors_without_the_opt_in(monkeypatch):
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    with pytest.raises(_lib.DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        Fd.FeatureBank(16).update(torch.zeros(4, 16))


def test_a_missing_bank_is_an_error_not_a_skipped_key(monkeypatch):
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    images = _u8(16, 3, 24, 20).permute(0, 2, 3, 1).contiguous()
    plain, kept = _metrics(), _metrics(keep_features=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain.update_uint8(images)
        kept.update_uint8(images)
    for flags in (dict(kid=True), dict(prc=True)):
        with pytest.raises(RuntimeError, match="keep_features"):
            plain.compute(splits=2, **flags)
        with pytest.raises(RuntimeError, match="real-side"):
            kept.compute(splits=2, **flags)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain.update_reference_uint8(images)                          # a real side alone does not help an object that kept no fake features
    with pytest.raises(RuntimeError, match="keep_features"):
        plain.compute(splits=2, prc=True)
    empty = _metrics(keep_features=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        empty.update_reference_uint8(images)
        empty.isc.update_logits(torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="fake-side"):
        empty.compute(splits=2, kid=True)
    assert sorted(plain.compute(splits=2)) == ["inception_score_mean", "inception_score_std"]


def test_compute_without_the_new_flags_returns_what_it_returned_before(monkeypatch, tmp_path):
    """The composition `compute()` was before `kid` / `prc` existed (the Inception Score of the logits, the Frechet distance of `statistics()` against the
    loaded file), spelled out here, equals today's result exactly, with and without kept features.  RECORDED holds what `compute()` returned on these inputs
    on a checkout of the parent commit, taken on the same machine and software as the first run of this test, where today's code returned the same three
    floats bit for bit; here they are held to 1e-9 relative, not to equality, because the score and the distance go through the host's BLAS and eigensolver,
    whose last bits may differ between CPUs."""
    from dmvae_amd.fid import frechet_distance
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    images = _u8(40, 3, 24, 20).permute(0, 2, 3, 1).contiguous()
    g = torch.Generator().manual_seed(5)
    a = torch.randn(16, 32, generator=g, dtype=torch.float64) * 0.2
    np.savez(tmp_path / "stats.npz", mu=(torch.randn(16, generator=g, dtype=torch.float64) * 0.1).numpy(), sigma=((a @ a.t()) / 32).numpy())
    results = []
    for keep in (False, True):
        m = _metrics(keep_features=keep)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for part in images.split(8):
                m.update_uint8(part)
        m.load_statistics_file(tmp_path / "stats.npz")
        out = m.compute(splits=5, rng_seed=2)
        mean, std = m.isc.compute(5, True, 2)
        mu, sigma, _ = m.statistics()
        assert out == {"inception_score_mean": mean, "inception_score_std": std, "frechet_inception_distance": float(frechet_distance(mu, sigma, *m.reference))}
        assert list(out) == ["inception_score_mean", "inception_score_std", "frechet_inception_distance"]
        results.append(out)
    assert results[0] == results[1]
    for key, want in RECORDED.items():
        assert abs(results[0][key] - want) <= 1e-9 * abs(want), (key, results[0][key])


RECORDED = {"inception_score_mean": 1.0458475560618328, "inception_score_std": 0.010349838835325776, "frechet_inception_distance": 0.3748187185748133}


# ---- two ranks over gloo ------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _two_sets():
    return _gauss(40, 16, 21), _gauss(48, 16, 22) * 1.1


def _values(m):
    return m.kid_values(3, 16, rng_seed=1).tolist(), m.precision_recall(3)


def _rank_worker(rank, world, port, q, real_file):
    torch.cuda.is_available = lambda: False                         # CPU ranks on every node
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), DMVAE_ALLOW_STOCK="1")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    warnings.simplefilter("ignore")
    from dmvae_amd import dist
    dist.init_distributed_mode(backend="gloo")
    fake, real = _two_sets()
    m = _metrics(keep_features=True)
    m.bank.update(fake[rank::world], torch.arange(40)[rank::world])             # sample_50k.py's interleaved indices
    m.update_reference_features(real[rank::world], torch.arange(48)[rank::world])
    first, second = _values(m), _values(m)
    # the real side as ONE file loaded on every rank: the whole set, not gathered again
    filed = _metrics(keep_features=True)
    filed.bank.update(fake[rank::world], torch.arange(40)[rank::world])
    filed.load_reference_features(real_file)
    from_file = _values(filed)
    # saving a sharded bank is a collective that writes the whole set once, from rank 0
    m.reference_bank.save(real_file + ".gathered.npz")
    dist.barrier()
    back = Fd.FeatureBank(16)
    back.load(real_file + ".gathered.npz")
    q.put((rank, first, second, len(m.bank), len(m.reference_bank), from_file, len(filed.reference_bank), sorted(back.index.tolist()), back.is_global))
    torch.distributed.destroy_process_group()


def test_banks_gather_rows_and_indices_over_two_ranks_gloo(monkeypatch, tmp_path):
    """Each rank holds every second row of either side; both ranks' subset values and precision / recall equal the single-process ones (KID bit for bit: the
    subsets follow the image indices, so the same rows meet in the same order), twice (the gather goes into temporaries).  The same with the real side
    loaded from one file on both ranks: a loaded bank is the whole set and is not gathered -- no row meets its own copy."""
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    fake, real = _two_sets()
    m = _metrics(keep_features=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.bank.update(fake)
        m.update_reference_features(real)
        whole = _values(m)
        m.reference_bank.save(tmp_path / "real.npz")
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, str(tmp_path / "real.npz"))) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[0] for r in res] == [0, 1] and [r[3:5] for r in res] == [(20, 24), (20, 24)]
    for _, first, second, _, _, from_file, n_filed, saved_index, saved_global in res:
        assert first == whole and second == whole
        assert from_file == whole and n_filed == 48
        assert saved_index == list(range(48)) and saved_global


def test_rows_that_meet_their_own_copy_are_refused(monkeypatch, tmp_path):
    """An image index twice among the rows -- what one set fed as a shard on every rank gathers to -- raises instead of shrinking every radius; a loaded bank
    takes no further rows; `.double()` / `.to(...)` move the banks' device and leave their dtypes; two sides on different devices are an error with a name."""
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    fake, real = _two_sets()
    m = _metrics(keep_features=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.bank.update(fake)
        m.isc.update_logits(torch.zeros(4, 8))
        m.update_reference_features(real)
        m.update_reference_features(real)                             # the same 48 rows again, default indices 48 .. 95: distinct images as far as anyone can tell
        assert len(m.reference_bank) == 96
        m.reference_bank.reset()
        m.update_reference_features(real, torch.arange(48))
        m.update_reference_features(real, torch.arange(48))          # the same indices twice
        for flags in (dict(kid=True, kid_subsets=2, kid_subset_size=16), dict(prc=True)):
            with pytest.raises(ValueError, match="more than once"):
                m.compute(splits=2, **flags)
        m.reference_bank.reset()
        m.update_reference_features(real)
        m.reference_bank.save(tmp_path / "real.npz")
        want = _values(m)
        m.load_reference_features(tmp_path / "real.npz")
        assert m.reference_bank.is_global and not m.bank.is_global and _values(m) == want
        with pytest.raises(ValueError, match="loaded from a file"):
            m.update_reference_features(real[:2])
        m.reference_bank.reset()
        assert not m.reference_bank.is_global
        m.update_reference_features(real)
        m.double()
        assert m.features_sum.dtype == torch.float64 and m.bank.features.dtype == torch.float32 and m.bank.index.dtype == torch.int64
        assert torch.equal(m.bank.features, fake) and _values(m) == want
        m.to("meta")
        assert m.bank.features.device.type == "meta" and m.reference_bank.features.device.type == "meta" and m.features_sum.device.type == "meta"
    other = _metrics(keep_features=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        other.bank.update(fake)
        other.update_reference_features(real)
        other.isc.update_logits(torch.zeros(4, 8))
    other.reference_bank._apply(lambda t: t.to("meta"))
    with pytest.raises(RuntimeError, match=r"\.to\(device\)"):
        other.compute(splits=2, prc=True)
