"""Not a test: the CPU restatement the FID tests compare against (tests/test_fid_cpu.py, tests/test_gpu_fid.py).

  * the f64 feature statistics and the elementwise bound any f64 summation order meets;
  * the bicubic resize + uint8 quantisation of evaluation/fid.py:61-64 from its formula -- the source coordinate in f32 as ATen computes it, everything after it
    in f64 --, with the rounding sites of the two input dtypes applied explicitly and a mask of the pixels whose result does not depend on the last bits of an
    f32 evaluation;
  * the Frechet distance through the symmetric form tr sqrt(s1 s2) = sum sqrt(eigvalsh(s1^1/2 s2 s1^1/2)), which shares no step with the eigvals route of
    dmvae_amd.fid.frechet_distance."""
import numpy as np
import torch

A = -0.75
F32_LEVEL_MARGIN = 2e-3        # f32 images: unstable within this many uint8 levels of an integer (7.8e-6 in value)
BF16_MIDPOINT_MARGIN = 8e-6    # bf16 images: unstable within this distance (in value) of a bf16 rounding midpoint
# both are four to five times the largest difference between ATen's f32 evaluation and this f64 one that was measured on the CPU, 1.75e-6


# ---- statistics -----------------------------------------------------------------------------------------------------------------------
def accumulate(x: torch.Tensor):
    """-> (sum, cov_sum) of features x [N, F] in f64."""
    xd = x.detach().cpu().double()
    return xd.sum(0), xd.t() @ xd


def accumulate_bound(x: torch.Tensor, n_total=None):
    """Elementwise error bounds (sum, cov_sum): 8 * N * 2^-53 * sum |terms| -- N 2^-53 sum |a b| holds for any order of an f64 sum of N terms; the factor 8
    covers the fused products of the matrix instruction and the add to the previous state."""
    xa = x.detach().cpu().double().abs()
    n = xa.shape[0] if n_total is None else n_total
    u = 8.0 * n * 2.0 ** -53
    return u * xa.sum(0), u * (xa.t() @ xa)


# ---- resize + quantise ----------------------------------------------------------------------------------------------------------------
def _c1(x):
    return ((A + 2) * x - (A + 3)) * x * x + 1


def _c2(x):
    return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A


def _taps(in_size: int, out_size: int):
    """-> (idx int64 [out, 4] clamped to the edge, weights f64 [out, 4]); scale, source coordinate, floor and fraction in f32."""
    scale = np.float32(in_size) / np.float32(out_size)
    o = np.arange(out_size, dtype=np.float32)
    src = (scale * (o + np.float32(0.5))).astype(np.float32) - np.float32(0.5)
    assert src.dtype == np.float32
    fl = np.floor(src)
    t = (src - fl).astype(np.float64)
    idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, in_size - 1)
    w = np.stack([_c2(t + 1), _c1(t), _c1(1 - t), _c2(2 - t)], axis=1)
    return idx, w


def resize_f64(img: torch.Tensor, size: int) -> np.ndarray:
    """img [B, C, H, W] -> f64 [B, C, size, size]: rows first (each source row interpolated along W), then the column combination; H == W == size: the image."""
    x = img.detach().cpu().double().numpy()
    h, w = x.shape[-2:]
    if h == size and w == size:
        return x
    ix, wx = _taps(w, size)
    iy, wy = _taps(h, size)
    rows = (x[..., ix] * wx).sum(-1)                        # [B, C, H, size]
    return (rows[..., iy, :] * wy[:, :, None]).sum(-2)      # [B, C, size(oy), 4, size(ox)] summed over the taps


def _to_bf16(v: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16).double().numpy()


def _bf16_midpoint_distance(v: np.ndarray) -> np.ndarray:
    """Distance from |v| to the nearest midpoint between two neighbouring bf16 values (8 significant bits); inf at 0."""
    a = np.abs(v)
    with np.errstate(divide="ignore"):
        ulp = np.exp2(np.floor(np.log2(a)) - 7)
    q = np.where(a > 0, a / np.where(a > 0, ulp, 1.0), 0.0)
    return np.where(a > 0, np.abs(q - np.floor(q) - 0.5) * ulp, np.inf)


def resize_u8(img: torch.Tensor, size: int):
    """-> (uint8 [B, C, size, size], stable bool mask).  img f32: trunc(clamp(v * 255)) of the f64 value v.  img bf16: v rounded to bf16, the product with
    255 rounded to bf16, clamp, trunc.  A pixel is stable when no evaluation within the margins above can land on another level."""
    v = resize_f64(img, size)
    if img.dtype == torch.bfloat16:
        stable = _bf16_midpoint_distance(v) >= BF16_MIDPOINT_MARGIN
        levels = _to_bf16(_to_bf16(v) * 255.0)              # the product of two 8-bit significands is exact in f64: one rounding
    else:
        assert img.dtype == torch.float32
        levels = v * 255.0
        stable = (np.abs(levels - np.round(levels)) >= F32_LEVEL_MARGIN) | (levels >= 255 + F32_LEVEL_MARGIN) | (levels <= -F32_LEVEL_MARGIN)
    u8 = np.floor(np.clip(levels, 0.0, 255.0)).astype(np.uint8)
    return torch.from_numpy(u8), torch.from_numpy(stable)


def check_resize(got: torch.Tensor, img: torch.Tensor, size: int):
    """The criterion of the resize tests -> (unstable share, mismatches at unstable pixels); asserts what must hold."""
    want, stable = resize_u8(img, size)
    got = got.cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape
    diff = (got.to(torch.int16) - want.to(torch.int16)).abs()
    share = 1.0 - stable.double().mean().item()
    print(f"resize {tuple(img.shape)} {img.dtype} -> {size}: unstable share {share:.4f}, stable mismatches {int((diff[stable] != 0).sum())}, "
          f"unstable mismatches {int((diff[~stable] != 0).sum())}, max |diff| {int(diff.max())}")
    assert share <= 0.10, share                              # a condition on the case, not a tolerance
    assert int((diff[stable] != 0).sum()) == 0
    assert int(diff.max()) <= 1
    return share, int((diff[~stable] != 0).sum())


# ---- Frechet distance -----------------------------------------------------------------------------------------------------------------
def frechet(mu1, s1, mu2, s2) -> float:
    mu1, s1, mu2, s2 = (np.asarray(torch.as_tensor(t).detach().cpu().double().numpy()) for t in (mu1, s1, mu2, s2))
    w, q = np.linalg.eigh((s1 + s1.T) / 2)
    h = (q * np.sqrt(np.clip(w, 0, None))) @ q.T
    m = h @ s2 @ h
    ev = np.linalg.eigvalsh((m + m.T) / 2)
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.clip(ev, 0, None)).sum())


def mean_cov(x: torch.Tensor):
    """Sample mean and unbiased covariance of features [N, F] in f64, from the centred data (not from the sums)."""
    xd = x.detach().cpu().double()
    mu = xd.mean(0)
    c = xd - mu
    return mu, c.t() @ c / (xd.shape[0] - 1)


def fid_from_features(real: torch.Tensor, fake: torch.Tensor) -> float:
    return frechet(*mean_cov(real), *mean_cov(fake))
