"""The sampler's evaluation tail on the MI355X (-m gpu): the TF1 bilinear resize kernel against the numpy restatement of tests/fidelity_spec.py bit for bit,
the Inception Score kernels against the f64 spec under `isc_bound` (a bound any summation order meets, derived there), their order-table and rerun
identities, and dmvae_amd.fidelity's two objects and `SamplePipeline.run(metrics=...)` around a stub extractor.

The figures observed on an MI355X are in the docstrings of the tests that print them."""
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import fidelity_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


# ---- resize ------------------------------------------------------------------------------------------------------------------------------------
def _u8(b, c, h, w, seed=0):
    return torch.randint(0, 256, (b, c, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(1000 * h + w + seed))


@pytest.mark.parametrize("h,w,s", [(1, 1, 4), (5, 7, 9), (8, 8, 8), (37, 23, 11), (16, 16, 299), (64, 48, 299), (256, 256, 299)])
@pytest.mark.parametrize("nhwc", [True, False])
def test_resize_equals_the_spec_bit_for_bit(h, w, s, nhwc):
    """B = 2, C = 3: one block and many, up and down, an odd size on each axis; both layouts.  At h == w == s the rule is the identity: (u8 - 128) / 128."""
    from dmvae_amd import ops
    x = _u8(2, 3, h, w)
    src = x.permute(0, 2, 3, 1).contiguous() if nhwc else x
    got = ops.resize_tf1_bilinear(src.to(DEV), s, nhwc=nhwc)
    assert got.shape == (2, 3, s, s) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), torch.from_numpy(S.resize_tf1_bilinear(src.numpy(), s, nhwc=nhwc)))
    if h == w == s:
        assert torch.equal(got.cpu(), (x.float() - 128) / 128)


def test_resize_one_plane_inside_a_sentinel_buffer_and_rerun():
    """C = 1, B = 1, 13 x 9 -> 21: the output sits inside a larger buffer filled with a sentinel, which is untouched afterwards; a second run gives the same
    bits."""
    from dmvae_amd import ops
    x = _u8(1, 1, 13, 9)
    want = torch.from_numpy(S.resize_tf1_bilinear(x.numpy(), 21, nhwc=False))
    pad, n = 512, 21 * 21
    runs = []
    for _ in range(2):
        big = torch.full((n + 2 * pad,), -7.25, device=DEV)
        out = ops.resize_tf1_bilinear(x.to(DEV), 21, nhwc=False, out=big[pad:pad + n].view(1, 1, 21, 21))
        assert out.data_ptr() == big.data_ptr() + 4 * pad
        assert (big[:pad] == -7.25).all() and (big[pad + n:] == -7.25).all()
        runs.append(big.cpu())
    assert torch.equal(runs[0][pad:pad + n].view(1, 1, 21, 21), want) and torch.equal(runs[0], runs[1])
    # the same plane as NHWC with C = 1 is the same memory
    assert torch.equal(ops.resize_tf1_bilinear(x.view(1, 13, 9, 1).to(DEV), 21, nhwc=True).cpu(), want)


def test_resize_refuses_what_it_does_not_cover():
    from dmvae_amd import _lib, ops
    with pytest.raises(TypeError):
        ops.resize_tf1_bilinear(torch.zeros(1, 8, 8, 3, device=DEV), 4)
    with pytest.raises(ValueError, match="size"):
        ops.resize_tf1_bilinear(torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV), 0)
    with pytest.raises(_lib.DmvaeHipError):
        ops.resize_tf1_bilinear(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 4)
    with pytest.raises(ValueError):
        ops.resize_tf1_bilinear(torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV), 4, out=torch.zeros(1, 3, 5, 5, device=DEV))


# ---- Inception Score -------------------------------------------------------------------------------------------------------------------------------
def _logits(n, classes, scale, dtype, shift=0.0, seed=0):
    """-> (x [n, classes] of `dtype` on the CPU, the same values on the device as a view with row pitch classes + 8 of a buffer with four more rows, NaN
    everywhere outside the view)."""
    g = torch.Generator().manual_seed(100 * n + classes + seed)
    x = (torch.randn(n, classes, generator=g, dtype=torch.float64) * scale + shift).to(dtype)
    buf = torch.full((n + 4, classes + 8), float("nan"), dtype=dtype)
    buf[:n, :classes] = x
    return x, buf.to(DEV)[:n, :classes]


def _check(got, x, order, splits, what):
    want, bound = S.inception_score(x.double().numpy(), order, splits), S.isc_bound(x.double().numpy(), order, splits)
    got = got.cpu().numpy()
    assert got.shape == (splits,) and got.dtype == np.float64 and np.isfinite(got).all() and (bound < 1e-9).all()
    ratio = (np.abs(got - want) / want / bound).max()
    print(f"inception score {what}: worst error / bound {ratio:.4f} (bound {bound.max():.2e})")
    assert ratio <= 1.0
    return want, bound


IS_SHAPES = [(10, 8, 10, 1), (23, 1008, 10, 3), (257, 1008, 10, 6), (64, 1000, 3, 30), (1000, 1008, 10, 4), (37, 5, 1, 100), (16, 2, 4, 1), (33, 1001, 3, 2)]


@pytest.mark.parametrize("n,classes,splits,scale", IS_SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, BF, torch.float64])
def test_inception_score_against_the_spec(n, classes, splits, scale, dtype):
    """|score - spec| <= isc_bound * score per split, the spec evaluated in f64 on the same (rounded) logits in the reference's per-row KL form.  The logits
    are a view (row pitch classes + 8, four more rows, NaN outside): a read past a row's classes or past row n shows as a NaN score.  With one row per split
    every score is 1 within the bound.  At (64, 1000, 3, 30) the same with 800 added to every logit, where an exp without the row maximum overflows f64.
    Observed on an MI355X, worst error / bound over the three dtypes: 0.014 at (16, 2, 4, 1), where the bound is 1.9e-14; 0.0011 at (64, 1000, 3, 30) + 800;
    at most 0.0003 at every other shape (bounds 5.6e-14 ... 1.2e-11)."""
    from dmvae_amd import ops
    x, xd = _logits(n, classes, scale, dtype)
    assert xd.stride() == (classes + 8, 1)
    got = ops.inception_score(xd, None, splits)
    _, bound = _check(got, x, None, splits, f"{(n, classes, splits, scale)} {dtype}")
    if n == splits:
        assert (np.abs(got.cpu().numpy() - 1.0) <= bound).all()
    if scale == 30:
        x8, x8d = _logits(n, classes, scale, dtype, shift=800.0)
        _check(ops.inception_score(x8d, None, splits), x8, None, splits, f"{(n, classes, splits, scale)} + 800 {dtype}")


@pytest.mark.parametrize("n,classes,splits,scale", [(23, 1008, 10, 3), (257, 1008, 10, 6), (37, 5, 1, 100), (33, 1001, 3, 2)])
def test_inception_score_order_table_and_rerun_identities(n, classes, splits, scale):
    """order=None == the identity table; a random permutation table == physically permuted rows with no table; a rerun == itself: all bit for bit.
    Observed on an MI355X: worst error / bound through a table 0.0001."""
    from dmvae_amd import ops
    x, xd = _logits(n, classes, scale, torch.float32)
    base = ops.inception_score(xd, None, splits)
    assert torch.equal(base, ops.inception_score(xd, torch.arange(n, device=DEV), splits))
    perm = torch.from_numpy(np.random.RandomState(n).permutation(n))
    got = ops.inception_score(xd, perm.to(DEV), splits)
    _check(got, x, perm.numpy(), splits, f"{(n, classes, splits, scale)} through a table")
    assert torch.equal(got, ops.inception_score(x[perm].to(DEV), None, splits))
    assert torch.equal(got, ops.inception_score(xd, perm.to(DEV), splits))
    assert splits == 1 or not torch.equal(got, base)                 # the table is really used: other rows in every split


def test_inception_score_refuses_a_table_out_of_range_before_any_launch():
    from dmvae_amd import _lib, ops
    _, xd = _logits(23, 1008, 3, torch.float32)
    lib, calls = _lib.lib(), []
    real = lib.dmvae_inception_score
    for bad in (23, -1):
        order = torch.arange(23, device=DEV)
        order[7] = bad
        lib.dmvae_inception_score = lambda *a: calls.append(a) or real(*a)
        try:
            with pytest.raises(ValueError, match="order"):
                ops.inception_score(xd, order, 10)
        finally:
            lib.dmvae_inception_score = real
    assert calls == []
    with pytest.raises(ValueError, match="splits"):
        ops.inception_score(xd, None, 24)
    with pytest.raises(TypeError):
        ops.inception_score(xd.half(), None, 10)
    with pytest.raises(TypeError):
        ops.inception_score(xd, torch.arange(23, device=DEV, dtype=torch.int32), 10)


# ---- InceptionScore object ---------------------------------------------------------------------------------------------------------------------------
def test_inception_score_object_batches_reverse_order_and_compute():
    """Updates of 1, 3, 17 and 236 rows (the buffer grows from 64 rows to 257) == one update of 257 rows, bit for bit; the rows given in reverse with their
    indices == the forward order, bit for bit; compute() == np.mean / np.std of the spec's scores within the bound.
    Observed on an MI355X: worst error / bound 0.0004 (bound 7.3e-12)."""
    from dmvae_amd.fidelity import InceptionScore
    x, _ = _logits(257, 1008, 6, torch.float32)
    xd = x.to(DEV)
    one, parts, rev = InceptionScore(), InceptionScore(), InceptionScore()
    one.update_logits(xd)
    for p in xd.split([1, 3, 17, 236]):
        parts.update_logits(p)
    idx = torch.arange(257, device=DEV)
    for p, i in zip(xd.flip(0).split([100, 157]), idx.flip(0).split([100, 157])):
        rev.update_logits(p, i)
    assert len(one) == len(parts) == len(rev) == 257 and torch.equal(parts.logits, xd) and torch.equal(rev.logits, xd.flip(0))
    for shuffle, seed in ((True, 0), (True, 3), (False, 0)):
        a = one.scores(10, shuffle, seed)
        assert a.dtype == torch.float64 and a.is_cuda
        assert torch.equal(a, parts.scores(10, shuffle, seed)) and torch.equal(a, rev.scores(10, shuffle, seed))
        order = S.row_order(np.arange(257), shuffle, seed)
        want, bound = _check(a, x, order, 10, f"object, shuffle {shuffle}, seed {seed}")
        mean, std = one.compute(10, shuffle, seed)
        assert abs(mean - np.mean(want)) <= bound.max() * np.mean(want) and abs(std - np.std(want)) <= 2 * bound.max() * want.max()
    assert not torch.equal(one.scores(10, True, 0), one.scores(10, True, 3))
    with pytest.raises(ValueError):
        InceptionScore(8).scores(10)
    one.reset()
    assert len(one) == 0


# ---- FidelityMetrics -----------------------------------------------------------------------------------------------------------------------------------
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


def _metrics(**kw):
    from dmvae_amd.fidelity import FidelityMetrics
    return FidelityMetrics(StubExtractor(), num_features=16, num_classes=8, eval_size=32, **kw).to(DEV)


def _same_state(a, b):
    return (a.num_samples == b.num_samples and torch.equal(a.features_sum, b.features_sum) and torch.equal(a.features_cov_sum, b.features_cov_sum)
            and torch.equal(a.isc.logits, b.isc.logits))


def _reference_statistics(path):
    g = torch.Generator().manual_seed(5)
    a = torch.randn(16, 32, generator=g, dtype=torch.float64) * 0.2
    mu, sigma = torch.randn(16, generator=g, dtype=torch.float64) * 0.1, (a @ a.t()) / 32
    np.savez(path, mu=mu.numpy(), sigma=sigma.numpy())
    return mu.numpy(), sigma.numpy()


def test_fidelity_metrics_end_to_end_with_a_stub_extractor(tmp_path):
    """40 uint8 images of 24 x 20 in batches of 8 through resize kernel -> stub -> both accumulators.  compute() against the spec evaluated on the CPU from the
    stub's own outputs (the device stub on the resize kernel's output, which equals the spec's bit for bit): the Inception Score within `isc_bound`, the FID
    against loaded statistics within 1e-6 relative (the tolerance of tests/test_gpu_fid.py's compute()).  update_folder over the same images as PNGs leaves every
    state bit-identical.  Observed on an MI355X: Inception Score worst error / bound 0.016 (bound 5.5e-14); FID 0.374818719973 on both sides."""
    from PIL import Image
    images = _u8(40, 3, 24, 20).permute(0, 2, 3, 1).contiguous()      # NHWC
    m = _metrics()
    stub, feats, logits = StubExtractor().to(DEV), [], []
    for part in images.split(8):
        m.update_uint8(part.to(DEV))
        x = torch.from_numpy(S.resize_tf1_bilinear(part.numpy(), 32)).to(DEV)
        f, l = stub(x)
        feats.append(f.cpu())
        logits.append(l.cpu())
    feats, logits = torch.cat(feats), torch.cat(logits)
    assert m.num_samples == 40 and torch.equal(m.isc.logits.cpu(), logits)
    out = m.compute(splits=5, rng_seed=2)
    assert sorted(out) == ["inception_score_mean", "inception_score_std"]
    order = S.row_order(np.arange(40), True, 2)
    want, bound = _check(m.isc.scores(5, True, 2), logits, order, 5, "FidelityMetrics")
    assert abs(out["inception_score_mean"] - np.mean(want)) <= bound.max() * np.mean(want)
    assert abs(out["inception_score_std"] - np.std(want)) <= 2 * bound.max() * want.max()
    mu, sigma = _reference_statistics(tmp_path / "stats.npz")
    m.load_statistics_file(tmp_path / "stats.npz")
    out = m.compute(splits=5, rng_seed=2)
    want_fid = S.fid_from_statistics(feats.numpy(), mu, sigma)
    print(f"FidelityMetrics FID: {out['frechet_inception_distance']:.12f}, spec {want_fid:.12f}, relative difference "
          f"{abs(out['frechet_inception_distance'] - want_fid) / want_fid:.3e}")
    assert sorted(out) == ["frechet_inception_distance", "inception_score_mean", "inception_score_std"]
    assert abs(out["frechet_inception_distance"] - want_fid) <= 1e-6 * want_fid
    os.makedirs(tmp_path / "png" / "sub")
    for i, a in enumerate(images.numpy()):
        Image.fromarray(a).save(tmp_path / "png" / ("sub" if i >= 32 else "") / f"{i:06d}.png")
    m2 = _metrics()
    assert m2.update_folder(tmp_path / "png", batch_size=8) == 40 and _same_state(m, m2) and torch.equal(m.isc.index, m2.isc.index)
    m2.load_statistics_file(tmp_path / "stats.npz")
    assert m2.compute(splits=5, rng_seed=2) == out


def test_sample_pipeline_feeds_the_metrics_from_device_memory(tmp_path):
    """run(max_iterations=2, metrics=m) on the smallest DiT / VAE of tests/test_gpu_sampler.py: the PNGs on disk, fed to a second FidelityMetrics by
    update_folder, give bit-identical states and scores; with write_png=False no file (and no folder) is written and the states are those of the same seeds."""
    from dmvae_amd.models.lightningdit import LightningDiT
    from dmvae_amd.models.vae import VAE
    from dmvae_amd.sample import SamplePipeline
    torch.manual_seed(4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = VAE(z_channels=32, model_size="base", encoder_kwargs=dict(embed_dim=256, depth=1, num_heads=4)).to(DEV).eval()
    dit = LightningDiT(input_size=16, patch_size=1, in_channels=32, hidden_size=192, depth=2, num_heads=3, num_classes=10).to(DEV).eval()
    with torch.no_grad():
        for blk in dit.blocks:
            blk.adaLN_modulation[1].weight.normal_(0, 0.02)
        dit.final_layer.linear.weight.normal_(0, 0.05)
    pipe = SamplePipeline(dit, vae, num_sampling_steps=4, latent_mean=0.0685, latent_scale=0.1763, time_dist_shift=2.5)
    kw = dict(per_proc_batch_size=5, num_fid_samples=40, num_classes=10, max_iterations=2)
    m = _metrics()
    torch.manual_seed(21)
    assert pipe.run(str(tmp_path / "a"), metrics=m, **kw) == 10
    assert sorted(os.listdir(tmp_path / "a")) == [f"{i:06d}.png" for i in range(5, 15)]
    assert m.num_samples == 10 and m.isc.index.tolist() == list(range(5, 15))
    folder = _metrics()
    assert folder.update_folder(tmp_path / "a", batch_size=5) == 10
    assert _same_state(m, folder) and torch.equal(m.isc.scores(2), folder.isc.scores(2))
    assert m.compute(splits=2) == folder.compute(splits=2)
    quiet = _metrics()
    torch.manual_seed(21)
    assert pipe.run(str(tmp_path / "b"), metrics=quiet, write_png=False, **kw) == 10
    assert not (tmp_path / "b").exists() and _same_state(m, quiet)
    with pytest.raises(ValueError, match="write_png"):
        pipe.run(str(tmp_path / "c"), write_png=False, **kw)


# ---- two ranks ---------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rccl_worker(rank, world, port, q):
    try:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch.distributed as tdist
        from dmvae_amd import dist
        from dmvae_amd.fidelity import InceptionScore
        dist.init_distributed_mode()                       # backend "nccl" = RCCL, one device per rank
        x, _ = _logits(40, 1008, 3, torch.float32)
        isc = InceptionScore()
        isc.update_logits(x[rank::world].to("cuda"), torch.arange(40)[rank::world])      # sample_50k.py's interleaved indices
        first, second = isc.scores(4, True, 1).tolist(), isc.scores(4, True, 1).tolist()
        dist.barrier()
        q.put((rank, first, second, len(isc), ""))
        tdist.destroy_process_group()
    except Exception as e:
        import traceback
        q.put((rank, None, None, -1, traceback.format_exc()[-1500:]))
        raise e


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two MI355X on one node (RCCL over xGMI)")
def test_scores_gather_rows_and_indices_over_two_gpus_rccl():
    """Each rank holds every second image on its own device; both ranks' scores() equal the single-process value bit for bit (the same rows in the same
    order), twice (the gather goes into temporaries)."""
    from dmvae_amd import ops
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rccl_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=120)
    x, _ = _logits(40, 1008, 3, torch.float32)
    whole = ops.inception_score(x.to(DEV), torch.from_numpy(S.row_order(np.arange(40), True, 1)).to(DEV), 4).tolist()
    for rank, first, second, n, tb in res:
        assert tb == "", tb
        assert n == 20 and first == whole and second == whole, rank
