"""SSIM on the CPU: the two facts csrc/ssim.hip is built on (the valid-filter witness equals torchmetrics' padded / cropped composition in f64, with or
without the variance clamp), the window against scipy's statement of it, dmvae_amd.metrics on CPU tensors behind the stock opt-in, `evaluate(..., ssim=True)`
and the --hip-metrics shadow.  The kernel itself is covered by tests/test_gpu_ssim.py, its entry points' validation by tests/test_ssim_abi.py."""
import os
import subprocess
import sys

import pytest
import torch

import ssim_spec as S
from conftest import ROOT

SHAPES = [s for s in S.SHAPES if s[2] * s[3] <= 64 * 64] + [(1, 3, 96, 80)]


@pytest.mark.parametrize("shape", SHAPES)
def test_witness_equals_the_literal_composition_in_f64(shape):
    """<= 1e-12 per image, clamped or not: the padding never reaches the cropped map, and the clamp is moot in f64.  The f32 composition's error is printed
    for the record only: 3e-7 ... 1.5e-6 on ordinary images; on the flat near-identical ones 3e-5 ... 7e-5 without the clamp and 1.3e-4 ... 4e-4 with it."""
    for name, a, b in S.cases(shape):
        want = S.ssim_valid(a, b)
        for clamp in (False, True):
            got = S.ssim_literal(a, b, clamp=clamp)
            assert got.dtype == torch.float64 and (got - want).abs().max().item() <= 1e-12, (name, clamp, (got - want).abs().max().item())
        e32 = [(S.ssim_literal(a, b, dtype=torch.float32, clamp=c).double() - want).abs().max().item() for c in (False, True)]
        print(f"{shape} {name}: SSIM {want[0].item():+.9f}, literal f32 composition off by {e32[0]:.2e} (clamped: {e32[1]:.2e})")


def test_known_values():
    """Zeros against ones: both variances and the covariance vanish, mu_p mu_t = 0: c1 / (1 + c1) = 9.999e-5.  An image against itself: 1."""
    z, o = torch.zeros(1, 1, 16, 16), torch.ones(1, 1, 16, 16)
    assert abs(S.ssim_valid(z, o).item() - 1e-4 / (1 + 1e-4)) <= 1e-15
    x = torch.rand(2, 3, 20, 31, generator=torch.Generator().manual_seed(0))
    assert (S.ssim_valid(x, x) - 1).abs().max().item() <= 1e-15
    assert (S.ssim_valid(x, 1 - x) < -0.5).all()                       # anti-correlated: negative
    # data_range enters through c1, c2 only
    assert (S.ssim_valid(x, x * 0.5, data_range=2.0) - S.ssim_literal(x, x * 0.5, data_range=2.0)).abs().max().item() <= 1e-12


def test_window_means_against_scipy():
    """scipy.ndimage.gaussian_filter(sigma=1.5, mode='mirror', truncate=3.5) is an independent statement of the window: radius int(3.5 * 1.5 + 0.5) = 5,
    normalised exp(-x^2 / (2 sigma^2)), and 'mirror' is torch's 'reflect'.  Its interior, 5 pixels in from every side, is the valid filter."""
    ndimage = pytest.importorskip("scipy.ndimage")
    x = torch.rand(37, 53, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    full = torch.from_numpy(ndimage.gaussian_filter(x.numpy(), sigma=S.SIGMA, mode="mirror", truncate=3.5))
    err = (full[S.PAD:-S.PAD, S.PAD:-S.PAD] - S.valid_filter(x)).abs().max().item()
    print(f"window means against scipy: {err:.2e}")
    assert err <= 1e-14


# ---- dmvae_amd.metrics on CPU tensors ----------------------------------------------------------------------------------------------------------
def test_cpu_tensors_need_the_stock_opt_in(monkeypatch):
    from dmvae_amd import metrics
    from dmvae_amd._lib import DmvaeHipError
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    x = torch.rand(2, 3, 16, 16)
    with pytest.raises(DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        metrics.SSIM(x * 2 - 1, x * 2 - 1)
    with pytest.raises(DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        metrics.ssim01(x, x)


@pytest.mark.parametrize("shape", [(3, 2, 11, 75), (2, 3, 37, 53)])
def test_stock_route_matches_the_witness(shape, monkeypatch):
    import warnings
    from dmvae_amd import metrics
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=".*STOCK PyTorch modules.*")
        for name, a, b in S.cases(shape):
            got = metrics.ssim01(a, b)
            assert got.dtype == torch.float64 and got.shape == (shape[0],)
            assert (got - S.ssim_valid(a, b)).abs().max().item() <= 1e-12, name
            pa, pb = S.pm1(a), S.pm1(b)
            want = S.ssim_valid(S.to01(pa), S.to01(pb))
            per, mean = metrics.SSIM(pa, pb)                        # the reference's pair: per-image values [T] and their mean, f32 for f32 inputs
            assert per.dtype == torch.float32 and per.shape == (shape[0],) and mean.dtype == torch.float32 and mean.dim() == 0
            # one rounding of an f64 value within 1e-12 of the witness: half an f32 ulp below 1 is 2^-25
            assert (per.double() - want).abs().max().item() <= 2.0 ** -24 and abs(mean.double().item() - want.mean().item()) <= 2.0 ** -24, name
            assert torch.equal(mean, metrics.ssim01(S.to01(pa), S.to01(pb)).mean().float())
            bf = metrics.SSIM(pa.bfloat16(), pb.bfloat16())         # bf16: the value of SSIM(pred.float(), gt.float())
            ref = metrics.SSIM(pa.bfloat16().float(), pb.bfloat16().float())
            assert torch.equal(bf[0], ref[0]) and torch.equal(bf[1], ref[1])
        got = metrics.ssim01(a, b * 0.5, data_range=2.0)
        assert (got - S.ssim_valid(a, b * 0.5, data_range=2.0)).abs().max().item() <= 1e-12


def test_metrics_argument_errors_and_the_other_two_names(monkeypatch):
    from dmvae_amd import evaluate, metrics
    monkeypatch.setenv("DMVAE_ALLOW_STOCK", "1")
    x = torch.rand(2, 3, 16, 16)
    for bad in (torch.rand(2, 3, 10, 16), torch.rand(2, 3, 16, 10)):
        with pytest.raises(ValueError, match="at least 11"):
            metrics.ssim01(bad, bad)
    with pytest.raises(ValueError):
        metrics.ssim01(x, x[:1])
    with pytest.raises(ValueError):
        metrics.ssim01(x[0], x[0])
    for dr in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="data_range"):
            metrics.ssim01(x, x, data_range=dr)
    assert metrics.PSNR is evaluate.psnr
    with pytest.raises(NotImplementedError, match="AlexNet"):
        metrics.LPIPS(x, x)


# ---- evaluate(..., ssim=True) ------------------------------------------------------------------------------------------------------------------
class StubVAE(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def encode(self, x):
        return x * 0.5

    def decode(self, z):
        return (z * 1.9).clamp(-1, 1)


def test_evaluate_reports_ssim_only_when_asked(allow_stock):
    from dmvae_amd.evaluate import evaluate
    g = torch.Generator().manual_seed(5)
    imgs = torch.rand(8, 3, 24, 20, generator=g) * 2 - 1
    batches = [(b, torch.zeros(len(b), dtype=torch.long)) for b in imgs.split([1, 5, 2])]
    plain = evaluate(StubVAE(), batches, num_samples=10, device="cpu")
    with_ssim = evaluate(StubVAE(), batches, num_samples=10, device="cpu", ssim=True)
    assert "SSIM" not in plain and set(with_ssim) == set(plain) | {"SSIM"}
    assert all(with_ssim[k] == plain[k] for k in plain)
    rec = (imgs * 0.5 * 1.9).clamp(-1, 1)
    want = S.ssim_valid((rec + 1) / 2, (imgs + 1) / 2).sum().item() / 10          # the sum over the images divided by num_samples, PSNR's convention
    assert abs(with_ssim["SSIM"] - want) <= 1e-12


# ---- the opt-in shadow -------------------------------------------------------------------------------------------------------------------------
def test_hip_metrics_shadow_is_an_opt_in():
    """In a fresh interpreter: install_shadow(ref) leaves evaluation.metrics the reference's file; install_shadow(ref, metrics=True) -- and the command line's
    --hip-metrics / DMVAE_HIP_METRICS=1 -- make it dmvae_amd.metrics; evaluation.fid is not touched by it."""
    code = r"""
import sys, os, tempfile
sys.path.insert(0, %r)
import run_on_mi355x as L
ref = tempfile.mkdtemp()
os.makedirs(os.path.join(ref, "evaluation"))
open(os.path.join(ref, "evaluation", "__init__.py"), "w").close()
open(os.path.join(ref, "evaluation", "fid.py"), "w").write("class FID: marker = 'reference file'\n")
open(os.path.join(ref, "evaluation", "metrics.py"), "w").write("PSNR = SSIM = 'reference metrics'\n")
optin = sys.argv[1] == "1"
out = L.install_shadow(ref, metrics=True) if optin else L.install_shadow(ref)
sys.path.insert(0, ref)
from evaluation.metrics import PSNR, SSIM
from evaluation.fid import FID
import dmvae_amd.metrics as ours
assert FID.marker == 'reference file'
assert ("evaluation.metrics" in out) == optin and "evaluation.metrics" not in L.SHADOWS
assert (SSIM is ours.SSIM and PSNR is ours.PSNR) if optin else (SSIM == 'reference metrics')
print("shadow ok")
""" % ROOT
    for optin in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code, optin], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "shadow ok" in r.stdout, r.stderr[-2000:]
    launcher = os.path.join(ROOT, "run_on_mi355x.py")
    clean = {k: v for k, v in os.environ.items() if k != "DMVAE_HIP_METRICS"}
    for argv, e in ((["--hip-metrics", "--check"], clean), (["--hip-fid", "--hip-metrics", "--check"], clean), (["--check"], dict(clean, DMVAE_HIP_METRICS="1"))):
        r = subprocess.run([sys.executable, launcher] + argv, capture_output=True, text=True, timeout=300, env=e)
        assert r.returncode == 0 and "evaluation.metrics" in r.stdout and "dmvae_amd.metrics" in r.stdout, r.stderr[-2000:]
    r = subprocess.run([sys.executable, launcher, "--check"], capture_output=True, text=True, timeout=300, env=clean)
    assert r.returncode == 0 and "evaluation.metrics" not in r.stdout, r.stderr[-2000:]
