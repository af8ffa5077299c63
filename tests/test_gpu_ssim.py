"""SSIM on the MI355X (-m gpu): csrc/ssim.hip against the f64 valid-filter witness of tests/ssim_spec.py on the shapes that walk its tiling (one output pixel,
one output row, exactly one 32 x 16 tile, one past it in both directions, ragged tiles, several planes, the workload's 256 px) and the inputs that stress
its arithmetic (near-identical flat images above all), then identity, reads outside the images, determinism and the public layers above the kernel.

The bound, |err| <= 1e-9 per image: each window moment carries <= 22 roundings of terms <= 1 (2.4e-15); a variance is a difference of two such moments; the
two factors' denominators are >= c1 = 1e-4 and c2 = 9e-4, which gives ~1e-10 per pixel at the worst, and the bound leaves a factor 10 over it.  Two f64
summation orders differed by at most 3.6e-13 on the CPU.
Observed on an MI355X: see the docstring of test_kernel_against_the_witness."""
import functools

import pytest
import torch

import ssim_spec as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
BOUND = 1e-9


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype, from_pm1):
    """[(name, a, b, witness)]: a, b CPU tensors of `dtype` as the kernel gets them; the witness is fed the same f32-mapped values (bf16 widened first)."""
    out = []
    for name, a, b in S.cases(shape):
        if from_pm1:
            a, b = S.pm1(a), S.pm1(b)
        a, b = a.to(dtype), b.to(dtype)
        fa, fb = a.float(), b.float()
        if from_pm1:
            fa, fb = S.to01(fa), S.to01(fb)
        out.append((name, a, b, S.ssim_valid(fa, fb)))
    return out


CASES = [(s, torch.float32, pm) for s in S.SHAPES for pm in (False, True)] + \
        [(s, BF, pm) for s in ((1, 1, 27, 43), (2, 3, 37, 53), (2, 3, 256, 256)) for pm in (False, True)]


@pytest.mark.parametrize("shape,dtype,from_pm1", CASES, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_kernel_against_the_witness(shape, dtype, from_pm1):
    """Per image |ops.ssim - witness| <= 1e-9 on every input of ssim_spec.cases.
    Observed on an MI355X: the worst error over all shapes, dtypes and inputs is 1.42e-13, at (3, 2, 11, 75) f32 on the flat 0.7 image with 1e-3 noise
    (1.2e-13 ... 1.4e-13 on that input at every shape; 7e-14 ... 1.0e-13 for bf16); the ones-minus-1e-4 input stays below 6e-15, every other input below
    1e-15.  evaluate(..., ssim=True) gave the witness's 0.798941986603 to the last printed digit."""
    from dmvae_amd import ops
    worst = 0.0
    for name, a, b, want in _inputs(shape, dtype, from_pm1):
        got = ops.ssim(a.to(DEV), b.to(DEV), from_pm1=from_pm1)
        assert got.dtype == torch.float64 and got.shape == (shape[0],) and got.device.type == "cuda"
        err = (got.cpu() - want).abs().max().item()
        print(f"ssim {shape} {dtype} from_pm1={from_pm1} {name}: {want[0].item():+.12f}, worst error {err:.2e}")
        worst = max(worst, err)
        assert err <= BOUND, (name, err)
    print(f"ssim {shape} {dtype} from_pm1={from_pm1}: worst error over the inputs {worst:.2e}")


def test_known_values_and_data_range():
    from dmvae_amd import ops
    z, o = torch.zeros(2, 3, 37, 53, device=DEV), torch.ones(2, 3, 37, 53, device=DEV)
    assert (ops.ssim(z, o).cpu() - 1e-4 / (1 + 1e-4)).abs().max().item() <= 1e-15
    _, a, b, _ = _inputs((2, 3, 37, 53), torch.float32, False)[0]
    got = ops.ssim(a.to(DEV), (b * 0.5).to(DEV), data_range=2.0).cpu()
    assert (got - S.ssim_valid(a, b * 0.5, data_range=2.0)).abs().max().item() <= BOUND


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (1, 1, 27, 43), (2, 3, 37, 53), (2, 3, 256, 256)])
def test_identical_images_give_one(shape, dtype):
    """|SSIM - 1| <= 1e-15 (not exact equality: mu^2 + mu^2 and 2 mu mu may contract differently)."""
    from dmvae_amd import ops
    for name, a, _, _ in _inputs(shape, dtype, False)[:2] + _inputs(shape, dtype, False)[4:]:
        x = a.to(DEV)
        for pm in (False, True):
            got = ops.ssim(x, x.clone(), from_pm1=pm).cpu()
            assert (got - 1).abs().max().item() <= 1e-15, (name, pm, (got - 1).abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("shape", [(3, 2, 11, 75), (1, 1, 27, 43), (2, 3, 37, 53)])
def test_nothing_outside_the_images_is_read_or_written(shape, dtype):
    """The images are the slice [1 : 1 + B] of a [B + 2, C, H, W] buffer of NaN; the workspace and `out` hold two more images' worth of NaN than the call
    covers.  Every output is finite (and the witness's), every NaN beyond B is still there."""
    from dmvae_amd import _lib
    b, c, h, w = shape
    lib = _lib.lib()
    _, a, t, want = _inputs(shape, dtype, False)[0]
    bufs = []
    for x in (a, t):
        buf = torch.full((b + 2, c, h, w), float("nan"), dtype=dtype)
        buf[1:1 + b] = x
        bufs.append(buf.to(DEV))
    va, vt = bufs[0][1:1 + b], bufs[1][1:1 + b]
    assert va.is_contiguous() and vt.is_contiguous()
    per = lib.dmvae_ssim_workspace(1, c, h, w) // 8
    assert lib.dmvae_ssim_workspace(b, c, h, w) == b * per * 8
    ws = torch.full(((b + 2) * per,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((b + 2,), float("nan"), dtype=torch.float64, device=DEV)
    rc = lib.dmvae_ssim(va.data_ptr(), vt.data_ptr(), int(dtype == BF), b, c, h, w, 0, 1.0, ws.data_ptr(), out.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.dmvae_last_error()
    ws, out = ws.cpu(), out.cpu()
    assert torch.isfinite(out[:b]).all() and torch.isfinite(ws[:b * per]).all()
    assert torch.isnan(out[b:]).all() and torch.isnan(ws[b * per:]).all()
    assert (out[:b] - want).abs().max().item() <= BOUND


def test_reruns_and_batches_give_the_same_bits():
    """Two runs give the same bits, and each image's value in a batch of 5 equals, bit for bit, its value when run alone."""
    from dmvae_amd import ops
    for name, a, b, _ in _inputs((5, 3, 64, 64), torch.float32, False):
        a, b = a.to(DEV), b.to(DEV)
        first, second = ops.ssim(a, b), ops.ssim(a, b)
        assert torch.equal(first, second), name
        alone = torch.cat([ops.ssim(a[i:i + 1], b[i:i + 1]) for i in range(5)])
        assert torch.equal(first, alone), name


def test_ops_ssim_refuses_what_it_does_not_cover():
    from dmvae_amd import _lib, ops
    x = torch.zeros(2, 3, 16, 16, device=DEV)
    with pytest.raises(TypeError):
        ops.ssim(x, x.bfloat16())
    with pytest.raises(TypeError):
        ops.ssim(x.half(), x.half())
    with pytest.raises(ValueError):
        ops.ssim(x, x[:1])
    with pytest.raises(ValueError):
        ops.ssim(x[0], x[0])
    with pytest.raises(ValueError):
        ops.ssim(x[:0], x[:0])
    with pytest.raises(ValueError, match="contiguous"):
        ops.ssim(x.transpose(2, 3), x.transpose(2, 3))
    with pytest.raises(_lib.DmvaeHipError, match="11"):
        ops.ssim(x[..., :10].contiguous(), x[..., :10].contiguous())
    with pytest.raises(_lib.DmvaeHipError, match="data_range"):
        ops.ssim(x, x, data_range=0.0)


# ---- through the public layers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_metrics_ssim_returns_the_references_pair(dtype):
    from dmvae_amd import metrics
    shape = (2, 3, 37, 53)
    for name, a, b, want in _inputs(shape, dtype, True):
        per, mean = metrics.SSIM(a.to(DEV), b.to(DEV))
        assert per.dtype == torch.float32 and per.shape == (2,) and mean.dtype == torch.float32 and mean.dim() == 0 and per.is_cuda and mean.is_cuda
        assert (per.cpu().double() - want).abs().max().item() <= BOUND + 2.0 ** -25          # one rounding to f32 of a value below 1
        assert abs(mean.item() - want.mean().item()) <= BOUND + 2.0 ** -25
        v01 = metrics.ssim01(S.to01(a.float()).to(DEV), S.to01(b.float()).to(DEV))
        assert v01.dtype == torch.float64 and (v01.cpu() - want).abs().max().item() <= BOUND
        assert torch.equal(mean, v01.mean().float()), name                                   # the mean is the per-image mean


class StubVAE(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def encode(self, x):
        return x * 0.5

    def decode(self, z):
        return (z * 1.9).clamp(-1, 1)


def test_ssim_as_a_metric_of_evaluate():
    """evaluate(..., ssim=True) adds "SSIM" = the witness's sum over the images / num_samples; every other key is bit-identical to a run without the flag."""
    from dmvae_amd.evaluate import evaluate
    g = torch.Generator().manual_seed(5)
    imgs = torch.rand(8, 3, 24, 20, generator=g) * 2 - 1
    batches = [(b, torch.zeros(len(b), dtype=torch.long)) for b in imgs.split([1, 5, 2])]
    vae = StubVAE().to(DEV)
    plain = evaluate(vae, batches, num_samples=10, device=DEV)
    with_ssim = evaluate(vae, batches, num_samples=10, device=DEV, ssim=True)
    assert "SSIM" not in plain and set(with_ssim) == set(plain) | {"SSIM"}
    assert all(with_ssim[k] == plain[k] for k in plain)
    rec = (imgs * 0.5 * 1.9).clamp(-1, 1)
    want = S.ssim_valid((rec + 1) / 2, (imgs + 1) / 2).sum().item() / 10
    print(f"evaluate: SSIM {with_ssim['SSIM']:.12f}, witness {want:.12f}")
    assert abs(with_ssim["SSIM"] - want) <= BOUND
