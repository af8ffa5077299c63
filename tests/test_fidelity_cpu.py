"""dmvae_amd.fidelity on the CPU: the numpy restatements of tests/fidelity_spec.py against the torch forms they restate (the index-select resize bit for bit,
the softmax / log_softmax loop within `isc_bound`), `row_order`, the two objects' host logic on the stock route behind DMVAE_ALLOW_STOCK=1, the two-rank gather
over gloo, and `SamplePipeline.run`'s new arguments.  The kernels themselves are covered by tests/test_gpu_fidelity.py."""
import os
import socket
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import fidelity_spec as S
from dmvae_amd import _lib
from dmvae_amd import fidelity as Fd

RESIZE_SHAPES = [(1, 1, 4), (5, 7, 9), (8, 8, 8), (37, 23, 11), (16, 16, 299), (256, 256, 299), (300, 301, 299)]


def _u8(b, c, h, w, seed=0):
    return torch.randint(0, 256, (b, c, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(1000 * h + w + seed))


def _torch_resize(x, size):
    """The index-select form on f32 tensors: x [B, C, H, W] f32 -> [B, C, size, size], not normalised."""
    h, w = x.shape[-2:]
    gy, gx = torch.arange(size, dtype=torch.float32) * (h / size), torch.arange(size, dtype=torch.float32) * (w / size)
    y0, x0 = gy.floor().long(), gx.floor().long()
    y1, x1 = torch.clamp(y0 + 1, max=h - 1), torch.clamp(x0 + 1, max=w - 1)
    dy, dx = (gy - y0.float()).view(1, 1, size, 1), (gx - x0.float()).view(1, 1, 1, size)
    tl, tr = x.index_select(2, y0).index_select(3, x0), x.index_select(2, y0).index_select(3, x1)
    bl, br = x.index_select(2, y1).index_select(3, x0), x.index_select(2, y1).index_select(3, x1)
    top = tl + (tr - tl) * dx
    bot = bl + (br - bl) * dx
    return top + (bot - top) * dy


@pytest.mark.parametrize("h,w,s", RESIZE_SHAPES)
def test_resize_spec_equals_the_index_select_form_bit_for_bit(h, w, s):
    u8 = _u8(2, 3, h, w)
    want = (_torch_resize(u8.float(), s) - 128) / 128
    assert np.array_equal(S.resize_tf1_bilinear(u8.numpy(), s, nhwc=False), want.numpy())
    assert np.array_equal(S.resize_tf1_bilinear(u8.permute(0, 2, 3, 1).contiguous().numpy(), s, nhwc=True), want.numpy())
    assert torch.equal(Fd._stock_resize_tf1_bilinear(u8, s, nhwc=False), want)
    if (h, w, s) == (8, 8, 8):
        assert torch.equal(want, (u8.float() - 128) / 128)


def _logits(n, classes, scale, seed=0, shift=0.0):
    g = torch.Generator().manual_seed(100 * n + classes + seed)
    return torch.randn(n, classes, generator=g) * scale + shift


def _torch_isc(x, splits):
    """The double loop over softmax / log_softmax on f64 tensors."""
    x = x.double()
    p, logp = x.softmax(dim=1), x.log_softmax(dim=1)
    n, out = x.shape[0], []
    for k in range(splits):
        pk, lk = p[k * n // splits:(k + 1) * n // splits], logp[k * n // splits:(k + 1) * n // splits]
        out.append((pk * (lk - pk.mean(dim=0, keepdim=True).log())).sum(dim=1).mean().exp().item())
    return np.asarray(out)


IS_SHAPES = [(10, 8, 10, 1), (23, 1008, 10, 3), (257, 1008, 10, 6), (64, 1000, 3, 30), (1000, 1008, 10, 4), (37, 5, 1, 100), (16, 2, 4, 1), (33, 1001, 3, 2)]


@pytest.mark.parametrize("n,classes,splits,scale", IS_SHAPES)
def test_isc_spec_equals_the_softmax_loop_within_the_bound(n, classes, splits, scale):
    x = _logits(n, classes, scale)
    got, want, bound = S.inception_score(x.numpy(), None, splits), _torch_isc(x, splits), S.isc_bound(x.numpy(), None, splits)
    assert got.shape == (splits,) and (bound < 1e-9).all()
    if n == splits:
        assert (np.abs(got - 1.0) <= bound).all()                     # one row per split: q = p, every score is 1
    finite = np.isfinite(want)                                        # the loop gives NaN where a probability underflows to 0 (0 * -inf); the spec's term is 0
    assert finite.all() or scale >= 30
    assert (np.abs(got - want)[finite] <= bound[finite] * want[finite]).all(), (np.abs(got - want) / want / bound).max()


def test_isc_spec_with_a_shift_a_max_free_exp_overflows_on():
    x = _logits(64, 1000, 30)
    a, b = S.inception_score(x.numpy(), None, 3), S.inception_score((x.double() + 800).numpy(), None, 3)
    assert np.isfinite(b).all() and (np.abs(a - b) <= (S.isc_bound(x.numpy(), None, 3) + S.isc_bound((x.double() + 800).numpy(), None, 3)) * a).all()


def test_row_order_properties():
    world, per = 4, 6
    index = np.concatenate([np.arange(per) * world + r for r in range(world)])      # rank-major gather of interleaved indices
    order = Fd.row_order(index, shuffle=False)
    assert order.dtype == np.int64 and np.array_equal(index[order], np.arange(world * per))
    assert np.array_equal(order, np.argsort(index, kind="stable")) and np.array_equal(order, S.row_order(index, False))
    for seed in (0, 7):
        got = Fd.row_order(index, True, seed)
        assert np.array_equal(got, Fd.row_order(index, True, seed)) and np.array_equal(got, S.row_order(index, True, seed))
        assert np.array_equal(index[got], np.random.RandomState(seed).permutation(world * per))
    assert not np.array_equal(Fd.row_order(index, True, 0), Fd.row_order(index, True, 7))
    assert np.array_equal(Fd.row_order(np.arange(9), True, 3), np.random.RandomState(3).permutation(9))


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


def test_objects_refuse_cpu_tensors_without_the_opt_in(monkeypatch):
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    with pytest.raises(_lib.DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        Fd.InceptionScore(8).update_logits(torch.zeros(4, 8))
    m = Fd.FidelityMetrics(StubExtractor(), num_features=16, num_classes=8, eval_size=32)
    with pytest.raises(_lib.DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        m.update_uint8(_u8(2, 3, 24, 20), nhwc=False)
    assert m.num_samples == 0 and len(m.isc) == 0


def test_inception_score_object_on_the_stock_route(monkeypatch):
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    x = _logits(57, 8, 2)
    index = torch.arange(57) * 3 + 5
    isc = Fd.InceptionScore(8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                               # the stock route announces itself once per process
        for part, idx in zip(x.flip(0).split([1, 3, 17, 36]), index.flip(0).split([1, 3, 17, 36])):      # reversed arrival, growing buffer
            isc.update_logits(part, idx)
    assert len(isc) == 57 and torch.equal(isc.logits, x.flip(0))
    for shuffle, seed in ((False, 0), (True, 0), (True, 5)):
        order = S.row_order(np.arange(57), shuffle, seed)             # by image index: the forward order, whatever the arrival
        want, bound = S.inception_score(x.numpy(), order, 10), S.isc_bound(x.numpy(), order, 10)
        got = isc.scores(10, shuffle, seed).numpy()
        assert (np.abs(got - want) <= bound * want).all()
        mean, std = isc.compute(10, shuffle, seed)
        assert abs(mean - np.mean(want)) <= bound.max() * np.mean(want) and abs(std - np.std(want)) <= 2 * bound.max() * want.max()
    with pytest.raises(ValueError):
        isc.scores(58)
    with pytest.raises(ValueError):
        isc.update_logits(torch.zeros(2, 9))
    isc.reset()
    assert len(isc) == 0
    with pytest.raises(ValueError):
        isc.scores(1)


def test_fidelity_metrics_on_the_stock_route_and_statistics_file(monkeypatch, tmp_path):
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    stub = StubExtractor()
    images = _u8(40, 3, 24, 20).permute(0, 2, 3, 1).contiguous()      # NHWC
    m = Fd.FidelityMetrics(stub, num_features=16, num_classes=8, eval_size=32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for part in images.split(8):
            m.update_uint8(part)
    assert m.num_samples == 40 and len(m.isc) == 40
    feats, logits = stub(torch.from_numpy(S.resize_tf1_bilinear(images.numpy(), 32)))
    out = m.compute(splits=5, rng_seed=3)
    assert sorted(out) == ["inception_score_mean", "inception_score_std"]      # no statistics loaded: no FID
    order = S.row_order(np.arange(40), True, 3)
    want, bound = S.inception_score(logits.numpy(), order, 5), S.isc_bound(logits.numpy(), order, 5)
    assert abs(out["inception_score_mean"] - np.mean(want)) <= bound.max() * np.mean(want)
    assert abs(out["inception_score_std"] - np.std(want)) <= 2 * bound.max() * want.max()
    # an npz of the reference's layout, written here
    g = torch.Generator().manual_seed(5)
    a = torch.randn(16, 32, generator=g, dtype=torch.float64)
    mu, sigma = torch.randn(16, generator=g, dtype=torch.float64) * 0.1, (a @ a.t()) / 32
    path = tmp_path / "stats.npz"
    np.savez(path, mu=mu.numpy(), sigma=sigma.numpy())
    m.load_statistics_file(path)
    assert torch.equal(m.reference[0], mu) and torch.equal(m.reference[1], sigma)
    out = m.compute(splits=5, rng_seed=3)
    assert sorted(out) == ["frechet_inception_distance", "inception_score_mean", "inception_score_std"]
    want_fid = S.fid_from_statistics(feats.numpy(), mu.numpy(), sigma.numpy())
    assert abs(out["frechet_inception_distance"] - want_fid) <= 1e-6 * want_fid
    np.savez(tmp_path / "bad.npz", mu=np.zeros(8), sigma=np.zeros((8, 8)))
    with pytest.raises(ValueError):
        m.load_statistics_file(tmp_path / "bad.npz")
    m.reset()
    assert m.num_samples == 0 and len(m.isc) == 0 and not m.features_cov_sum.any() and m.reference is not None
    with pytest.raises(ValueError):
        Fd.FidelityMetrics(stub, num_features=24)


def test_update_folder_feeds_the_same_path(monkeypatch, tmp_path):
    from PIL import Image
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    images = _u8(12, 3, 24, 20, seed=2).permute(0, 2, 3, 1).contiguous()
    os.makedirs(tmp_path / "sub")
    for i, a in enumerate(images.numpy()):
        Image.fromarray(a).save(tmp_path / ("sub" if i >= 8 else "") / f"{i:06d}.png")
    (tmp_path / "notes.txt").write_text("not an image")
    a, b = (Fd.FidelityMetrics(StubExtractor(), num_features=16, num_classes=8, eval_size=32) for _ in range(2))
    for part in images.split(4):
        a.update_uint8(part)
    assert b.update_folder(tmp_path, batch_size=4) == 12
    assert torch.equal(a.features_sum, b.features_sum) and torch.equal(a.features_cov_sum, b.features_cov_sum)
    assert torch.equal(a.isc.logits, b.isc.logits) and torch.equal(a.isc.index, b.isc.index) and a.compute(3) == b.compute(3)


def test_sample_pipeline_run_without_png_needs_metrics(tmp_path):
    from dmvae_amd.sample import SamplePipeline
    pipe = SamplePipeline(None, None, num_sampling_steps=2)
    with pytest.raises(ValueError, match="write_png"):
        pipe.run(str(tmp_path / "out"), write_png=False)
    assert not (tmp_path / "out").exists()


# ---- two ranks over gloo ------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, q):
    torch.cuda.is_available = lambda: False                         # CPU ranks on every node
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), DMVAE_ALLOW_STOCK="1")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    warnings.simplefilter("ignore")
    from dmvae_amd import dist
    dist.init_distributed_mode(backend="gloo")
    x = _logits(40, 8, 2)
    isc = Fd.InceptionScore(8)
    isc.update_logits(x[rank::world], torch.arange(40)[rank::world])            # sample_50k.py's interleaved indices
    first, second = isc.scores(4, True, 1).tolist(), isc.scores(4, True, 1).tolist()
    dist.barrier()
    q.put((rank, first, second, len(isc)))
    torch.distributed.destroy_process_group()


def test_scores_gather_rows_and_indices_over_two_ranks_gloo():
    """Each rank holds every second image; both ranks' scores() equal the single-process value, twice (the gather goes into temporaries)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    x = _logits(40, 8, 2)
    whole = Fd._stock_inception_score(x, torch.from_numpy(S.row_order(np.arange(40), True, 1)), 4).tolist()
    assert [r[0] for r in res] == [0, 1] and [r[3] for r in res] == [20, 20]
    for _, first, second, _ in res:
        assert first == whole and second == whole                   # the same rows in the same order: the same bits
