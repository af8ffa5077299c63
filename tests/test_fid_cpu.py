"""dmvae_amd.fid on the CPU: the Frechet distance against closed forms, `compute()` from loaded states against tests/fid_spec.py, the protocol's host
logic (save / load, statistics, reset, the errors), the cross-rank sum over gloo, the two entry points' argument validation and the --hip-fid shadow.
The kernels themselves are covered by tests/test_gpu_fid.py."""
import ctypes
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

import fid_spec as S
from conftest import ROOT
from dmvae_amd.fid import FID, frechet_distance


class Stub(torch.nn.Module):
    """A feature extractor that is never called: the CPU tests feed features or states."""

    def __init__(self, num_features=64):
        super().__init__()
        self.num_features = num_features

    def forward(self, u8):
        raise AssertionError("the extractor is not part of these tests")


def _spd(f, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(f, 2 * f, generator=g, dtype=torch.float64)
    return scale * (a @ a.t()) / (2 * f)


def _features(n, f, seed, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    mix = torch.randn(f, f, generator=g, dtype=torch.float64) / f ** 0.5
    return (torch.randn(n, f, generator=g, dtype=torch.float64) @ mix + shift).float()


def _loaded(real_x, fake_x, **kw):
    """An FID whose states are the spec's f64 sums of the two feature sets (no accumulation code runs)."""
    fid = FID(Stub(real_x.shape[1]), **kw)
    for real, x in ((True, real_x), (False, fake_x)):
        s, c = S.accumulate(x)
        fid._set("real" if real else "fake", s, c, x.shape[0])
    return fid


def _tol(real, fake):
    """Bound for comparing two evaluations of the FID of feature sets with fewer samples than features (N2 = 37 < F = 64: the covariances are singular).
    Well-conditioned part: 1e-9 * (tr s1 + tr s2), as for the closed forms.  Singular part: s1 s2 has z = F - (min(N1, N2) - 1) zero eigenvalues, which any
    f64 route computes as numbers of size e = F * 2^-53 * |s1|_2 |s2|_2 and either sign; the square root turns each into up to sqrt(e) -- 3e-7 here, not
    1e-16 -- in the trace term, which enters the value twice, in each of the two evaluations compared: 4 z sqrt(e)."""
    s1, s2 = S.mean_cov(real)[1], S.mean_cov(fake)[1]
    f = s1.shape[0]
    z = max(f - (min(real.shape[0], fake.shape[0]) - 1), 0)
    e = f * 2.0 ** -53 * torch.linalg.matrix_norm(s1, 2).item() * torch.linalg.matrix_norm(s2, 2).item()
    return 1e-9 * (s1.trace().item() + s2.trace().item()) + 4 * z * e ** 0.5


@pytest.mark.parametrize("f", [64, 2048])
def test_frechet_distance_against_closed_forms(f):
    """Identical statistics -> 0, equal covariances -> |dmu|^2, diagonal covariances -> sum (mu1 - mu2)^2 + sum (sqrt a - sqrt b)^2, each within
    1e-9 * (tr s1 + tr s2).  Residuals seen on the CPU build: F = 64: -9.9e-14 (identical), -9.9e-14 (shifted), 0 (diagonal) on traces of 124.3 / 124.3 / 102.5;
    F = 2048: -5.9e-12 (identical), -5.9e-12 (shifted), -4.5e-12 (diagonal) on traces of 4092 / 4092 / 3077 -- six orders below the bound of 4.1e-6."""
    g = torch.Generator().manual_seed(f)
    mu, sig = torch.randn(f, generator=g, dtype=torch.float64), _spd(f, 1)
    tol = 1e-9 * 2 * sig.trace().item()
    r0 = frechet_distance(mu, sig, mu, sig)
    assert r0.dim() == 0 and r0.dtype == torch.float64
    assert abs(r0.item()) <= tol
    d = torch.randn(f, generator=g, dtype=torch.float64)
    r1 = frechet_distance(mu, sig, mu + d, sig).item() - d.dot(d).item()
    assert abs(r1) <= tol
    a, b = torch.rand(f, generator=g, dtype=torch.float64) + 0.25, torch.rand(f, generator=g, dtype=torch.float64) + 0.25
    want = d.dot(d).item() + (a.sqrt() - b.sqrt()).pow(2).sum().item()
    r2 = frechet_distance(mu, torch.diag(a), mu + d, torch.diag(b)).item() - want
    print(f"F {f}: residuals {r0.item():.3e} {r1:.3e} {r2:.3e}, traces {2 * sig.trace().item():.1f} {(a.sum() + b.sum()).item():.1f}")
    assert abs(r2) <= 1e-9 * (a.sum() + b.sum()).item()


def test_compute_from_loaded_states_against_the_spec():
    """N1 = 50, N2 = 37, F = 64: mean and covariance from the sums, then the eigvals route, against the spec's centred covariance and symmetric route."""
    real, fake = _features(50, 64, 1), _features(37, 64, 2, shift=0.3)
    fid = _loaded(real, fake)
    got, want = fid.compute(), S.fid_from_features(real, fake)
    print(f"compute() {got.item():.12f}, spec {want:.12f}, difference {got.item() - want:.3e}, bound {_tol(real, fake):.3e}")
    assert got.dim() == 0 and abs(got.item() - want) <= _tol(real, fake), (got.item(), want)
    assert fid.compute().item() == got.item()                        # a second compute(): the same value, nothing counted twice
    assert int(fid.real_features_num_samples) == 50 and int(fid.fake_features_num_samples) == 37


def test_state_layout_is_the_references():
    fid = FID(Stub(32))
    want = {"real_features_sum": ((32,), torch.float64), "real_features_cov_sum": ((32, 32), torch.float64), "real_features_num_samples": ((), torch.int64),
            "fake_features_sum": ((32,), torch.float64), "fake_features_cov_sum": ((32, 32), torch.float64), "fake_features_num_samples": ((), torch.int64)}
    got = {k: (tuple(v.shape), v.dtype) for k, v in fid.named_buffers()}
    assert got == want
    assert fid.eval_size == 299 and fid.normalize is False and fid.reset_real_features is True


def test_save_load_and_statistics_round_trips(tmp_path):
    real, fake = _features(50, 64, 3), _features(37, 64, 4)
    a = _loaded(real, fake)
    a.save(True, tmp_path / "real.pt")
    a.save(False, tmp_path / "fake.pt")
    d = torch.load(tmp_path / "real.pt", map_location="cpu")
    assert sorted(d) == ["real_features_cov_sum", "real_features_num_samples", "real_features_sum"]      # evaluation/fid.py:69-73
    assert sorted(torch.load(tmp_path / "fake.pt", map_location="cpu")) == ["fake_features_cov_sum", "fake_features_num_samples", "fake_features_sum"]
    b = FID(Stub(64))
    b.load(True, tmp_path / "real.pt")
    b.load(False, tmp_path / "fake.pt")
    for k, v in a.named_buffers():
        assert torch.equal(v, dict(b.named_buffers())[k]), k
    assert b.compute().item() == a.compute().item()
    # a file as the reference's `save` writes it: the same keys around torchmetrics' states
    s, c = S.accumulate(real)
    torch.save({"real_features_sum": s, "real_features_cov_sum": c, "real_features_num_samples": torch.tensor(50)}, tmp_path / "theirs.pt")
    e = FID(Stub(64))
    e.load(True, tmp_path / "theirs.pt")
    assert torch.equal(e.real_features_cov_sum, c) and int(e.real_features_num_samples) == 50 and e.real_features_num_samples.dtype == torch.int64
    # statistics / load_statistics
    mu, sigma, n = a.statistics(True)
    mu_w, sigma_w = S.mean_cov(real)
    assert n == 50 and (mu - mu_w).abs().max() <= 1e-13 and (sigma - sigma_w).abs().max() <= 1e-12 * sigma_w.abs().max()
    c2 = FID(Stub(64))
    c2.load_statistics(True, mu.numpy(), sigma.numpy(), n)             # arrays, as an npz holds them
    c2.load_statistics(False, *a.statistics(False))
    mu2, sigma2, n2 = c2.statistics(True)
    assert n2 == 50 and (mu2 - mu).abs().max() <= 1e-14 and (sigma2 - sigma).abs().max() <= 1e-12 * sigma.abs().max()
    assert abs(c2.compute().item() - a.compute().item()) <= _tol(real, fake)
    with pytest.raises(ValueError):
        c2.load_statistics(True, mu[:32], sigma[:32, :32], n)


def test_fewer_than_two_samples_is_an_error():
    x = _features(5, 64, 5)
    for n_real, n_fake in ((5, 1), (1, 5), (0, 0)):
        fid = FID(Stub(64))
        for side, n in (("real", n_real), ("fake", n_fake)):
            if n:
                s, c = S.accumulate(x[:n])
                fid._set(side, s, c, n)
        with pytest.raises(RuntimeError, match="More than one sample"):
            fid.compute()


def test_reset_honours_reset_real_features():
    real, fake = _features(9, 64, 6), _features(7, 64, 7)
    keep = _loaded(real, fake, reset_real_features=False)
    real_sum = keep.real_features_sum.clone()
    keep.reset()
    assert torch.equal(keep.real_features_sum, real_sum) and int(keep.real_features_num_samples) == 9
    assert int(keep.fake_features_num_samples) == 0 and not keep.fake_features_sum.any() and not keep.fake_features_cov_sum.any()
    both = _loaded(real, fake)
    both.reset()
    assert all(not v.any() for v in both.buffers())


def test_int_feature_without_torchmetrics_is_an_import_error():
    try:
        import torchmetrics  # noqa: F401
        have = True
    except ImportError:
        have = False
    if not have:                      # with torchmetrics installed the int builds its network (and its weights): not this test's business
        with pytest.raises(ImportError, match=r"(?s)torchmetrics.*FID\(feature=module\)"):
            FID(2048)
    with pytest.raises(TypeError):
        FID("2048")
    with pytest.raises(ValueError, match="multiple of 16"):
        FID(Stub(40))
    with pytest.raises(ValueError, match="normalize"):
        FID(Stub(64), normalize=True)


def test_num_features_is_probed_on_a_zero_image():
    seen = []

    def extractor(u8):
        seen.append((u8.dtype, tuple(u8.shape), int(u8.max())))
        return torch.zeros(u8.shape[0], 48)

    fid = FID(extractor, eval_size=19)
    assert fid.num_features == 48 and seen == [(torch.uint8, (1, 3, 19, 19), 0)]


def test_cpu_tensors_need_the_stock_opt_in(monkeypatch):
    from dmvae_amd._lib import DmvaeHipError
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    fid = FID(Stub(64))
    with pytest.raises(DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        fid.update_features(_features(4, 64, 8), True)
    with pytest.raises(DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        fid.update(torch.rand(2, 3, 16, 16), False)
    assert int(fid.real_features_num_samples) == 0 and not fid.real_features_cov_sum.any()


def test_stock_route_accumulates_like_the_spec(allow_stock):
    """Behind the opt-in the CPU route is torchmetrics' composition: batches of 1, 5 and 2 per side, then the spec on the concatenation."""
    real, fake = _features(8, 64, 9), _features(8, 64, 10, shift=0.2)
    fid = FID(Stub(64))
    for x, side in ((real, True), (fake, False)):
        for part in x.split([1, 5, 2]):
            fid.update_features(part, side)
    s, c = S.accumulate(real)
    assert (fid.real_features_sum - s).abs().max() <= 1e-12 and (fid.real_features_cov_sum - c).abs().max() <= 1e-12 * c.abs().max()
    assert abs(fid.compute().item() - S.fid_from_features(real, fake)) <= _tol(real, fake)


# ---- two ranks over gloo ------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, q):
    torch.cuda.is_available = lambda: False                         # CPU ranks on every node
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from dmvae_amd import dist
    dist.init_distributed_mode(backend="gloo")
    real, fake = _features(50, 64, 1), _features(37, 64, 2, shift=0.3)
    fid = _loaded(real[rank::world], fake[rank::world])             # each rank holds the statistics of its half
    first, second = fid.compute().item(), fid.compute().item()
    dist.barrier()
    q.put((rank, first, second, int(fid.real_features_num_samples)))
    torch.distributed.destroy_process_group()


def test_compute_sums_the_states_over_two_ranks_gloo():
    """Each rank loads half of the statistics; both ranks' compute() give the single-process value, twice (the sum goes into temporaries)."""
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
    real, fake = _features(50, 64, 1), _features(37, 64, 2, shift=0.3)
    whole = _loaded(real, fake).compute().item()
    assert [r[0] for r in res] == [0, 1]
    for _, first, second, n_local in res:
        assert abs(first - whole) <= _tol(real, fake) and second == first
    assert [r[3] for r in res] == [25, 25]                           # the ranks' own states are untouched
    assert abs(whole - S.fid_from_features(real, fake)) <= _tol(real, fake)


# ---- the C ABI's argument validation ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    buf = [ctypes.create_string_buffer(64) for _ in range(3)]
    x, s, c = (ctypes.cast(b, ctypes.c_void_p) for b in buf)
    acc, rsz = lib.dmvae_fid_accumulate, lib.dmvae_fid_resize_u8
    for args in ((None, 0, 4, 16, 16, s, c), (x, 0, 4, 16, 16, None, c), (x, 0, 4, 16, 16, s, None)):
        assert acc(*args, None) == -22 and b"NULL" in lib.dmvae_last_error()
    for f in (0, 8, 24, 40, 4095, 4112, 8192, -16):
        assert acc(x, 0, 4, f, max(f, 16), s, c, None) == -22 and b"multiple of 16" in lib.dmvae_last_error(), f
    assert acc(x, 0, 0, 16, 16, s, c, None) == -22 and b"n > 0" in lib.dmvae_last_error()
    assert acc(x, 0, 4, 32, 16, s, c, None) == -22 and b"leading dimension" in lib.dmvae_last_error()
    assert acc(x, 3, 4, 16, 16, s, c, None) == -22 and b"x_dtype" in lib.dmvae_last_error()
    assert rsz(None, 0, 6, 16, 16, 19, s, None) == -22 and b"NULL" in lib.dmvae_last_error()
    assert rsz(x, 0, 6, 16, 16, 19, None, None) == -22 and b"NULL" in lib.dmvae_last_error()
    for size in (0, -1):
        assert rsz(x, 0, 6, 16, 16, size, s, None) == -22 and b"s >= 1" in lib.dmvae_last_error()
    for h, w, planes in ((0, 16, 6), (16, 0, 6), (16, 16, 0)):
        assert rsz(x, 1, planes, h, w, 19, s, None) == -22
    assert lib.dmvae_abi_version() == 9                              # two new entry points: a compatible extension


def test_ops_refuse_cpu_tensors():
    from dmvae_amd import _lib, ops
    with pytest.raises(_lib.DmvaeHipError):
        ops.fid_accumulate(torch.zeros(4, 16), torch.zeros(16, dtype=torch.float64), torch.zeros(16, 16, dtype=torch.float64))
    with pytest.raises(_lib.DmvaeHipError):
        ops.fid_resize_u8(torch.zeros(1, 3, 16, 16), 19)


# ---- the opt-in shadow -------------------------------------------------------------------------------------------------------------------
def test_hip_fid_shadow_is_an_opt_in():
    """In a fresh interpreter: install_shadow(ref) leaves evaluation.fid the reference's file, install_shadow(ref, fid=True) -- and the command line's
    --hip-fid / DMVAE_HIP_FID=1 -- make it dmvae_amd.fid; evaluation.metrics stays the reference's either way."""
    code = r"""
import sys, os, tempfile
sys.path.insert(0, %r)
import run_on_mi355x as L
ref = tempfile.mkdtemp()
os.makedirs(os.path.join(ref, "evaluation"))
open(os.path.join(ref, "evaluation", "__init__.py"), "w").close()
open(os.path.join(ref, "evaluation", "fid.py"), "w").write("class FID: marker = 'reference file'\n")
open(os.path.join(ref, "evaluation", "metrics.py"), "w").write("PSNR = 'reference metrics'\n")
optin = sys.argv[1] == "1"
out = L.install_shadow(ref, fid=True) if optin else L.install_shadow(ref)
sys.path.insert(0, ref)
from evaluation.fid import FID
from evaluation.metrics import PSNR
import dmvae_amd.fid as ours
assert PSNR == 'reference metrics'
assert ("evaluation.fid" in out) == optin and "evaluation.fid" not in L.SHADOWS
assert (FID is ours.FID) if optin else (FID.marker == 'reference file')
print("shadow ok")
""" % ROOT
    for optin in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code, optin], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "shadow ok" in r.stdout, r.stderr[-2000:]
    clean = {k: v for k, v in os.environ.items() if k != "DMVAE_HIP_FID"}
    for argv, e in ((["--hip-fid", "--check"], clean), (["--hip-dinodisc", "--hip-fid", "--check"], clean), (["--check"], dict(clean, DMVAE_HIP_FID="1"))):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "run_on_mi355x.py")] + argv, capture_output=True, text=True, timeout=300, env=e)
        assert r.returncode == 0 and "evaluation.fid" in r.stdout and "dmvae_amd.fid" in r.stdout, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_on_mi355x.py"), "--check"], capture_output=True, text=True, timeout=300, env=clean)
    assert r.returncode == 0 and "evaluation.fid" not in r.stdout, r.stderr[-2000:]
