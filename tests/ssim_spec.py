"""SSIM as evaluation/metrics.py:16-23 computes it (torchmetrics' StructuralSimilarityIndexMeasure at its defaults, reduction 'none'), restated twice in plain
torch on the CPU.  Nothing here imports dmvae_amd.

`ssim_valid`   the witness: a VALID 11 x 11 Gaussian filter over the raw images in f64, written as shifted slices (no conv2d, no padding), averaged over the
               (H - 10) x (W - 10) outputs.
`ssim_literal` the algorithm step by step: reflect-pad by 5, concatenate p, t, p p, t t, p t, one depthwise conv2d with the outer-product window, the moments,
               the SSIM map, crop 5 from every side, mean -- in a selectable dtype and with the variance clamp of newer torchmetrics optional.
The two agree to the noise between two f64 summation orders (tests/test_ssim_cpu.py): after the crop no surviving pixel's window touches the padding.

`cases` builds the inputs both test files use; everything is seeded and generated on the CPU."""
import torch
import torch.nn.functional as F

WIN, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
PAD = (WIN - 1) // 2

SHAPES = [(1, 1, 11, 11), (3, 2, 11, 75), (1, 1, 26, 42), (1, 1, 27, 43), (2, 3, 37, 53), (5, 3, 64, 64), (2, 3, 256, 256)]


def window(dtype=torch.float64):
    """g[i] = exp(-((i - 5) / 1.5)^2 / 2) / sum g, built in `dtype` the way torchmetrics builds it in the inputs' dtype."""
    d = torch.arange((1 - WIN) / 2, (1 + WIN) / 2, 1, dtype=dtype)
    g = torch.exp(-torch.pow(d / SIGMA, 2) / 2)
    return g / g.sum()


def _constants(data_range):
    return (K1 * data_range) ** 2, (K2 * data_range) ** 2


def valid_filter(x):
    """x [..., H, W] f64 -> [..., H - 10, W - 10]: sum_i sum_j g[i] g[j] x[y + i, x + j], rows of the window first, then its columns."""
    g = window()
    h, w = x.shape[-2:]
    rows = sum(g[k] * x[..., :, k:k + w - (WIN - 1)] for k in range(WIN))
    return sum(g[k] * rows[..., k:k + h - (WIN - 1), :] for k in range(WIN))


def ssim_valid(p, t, data_range=1.0):
    """The witness: per-image SSIM f64 [B] of p, t [B, C, H, W] (any float dtype, widened to f64 exactly), H, W >= 11."""
    p, t = p.double(), t.double()
    assert p.shape == t.shape and p.dim() == 4 and p.shape[-1] >= WIN and p.shape[-2] >= WIN
    c1, c2 = _constants(data_range)
    mp, mt, epp, ett, ept = (valid_filter(x) for x in (p, t, p * p, t * t, p * t))
    sp, st, spt = epp - mp * mp, ett - mt * mt, ept - mp * mt
    m = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (sp + st + c2))
    return m.reshape(m.shape[0], -1).mean(-1)


def ssim_literal(p, t, data_range=1.0, dtype=torch.float64, clamp=False):
    """The padded / cropped composition in `dtype` -> per-image values [B] in `dtype`."""
    p, t = p.to(dtype), t.to(dtype)
    b, c = p.shape[:2]
    c1, c2 = _constants(data_range)
    g = window(dtype).unsqueeze(0)
    kernel = torch.matmul(g.t(), g).expand(c, 1, WIN, WIN)
    p = F.pad(p, (PAD, PAD, PAD, PAD), mode="reflect")
    t = F.pad(t, (PAD, PAD, PAD, PAD), mode="reflect")
    out = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), kernel, groups=c).split(b)
    mpp, mtt, mpt = out[0].pow(2), out[1].pow(2), out[0] * out[1]
    sp, st, spt = out[2] - mpp, out[3] - mtt, out[4] - mpt
    if clamp:
        sp, st = torch.clamp(sp, min=0.0), torch.clamp(st, min=0.0)
    full = ((2 * mpt + c1) * (2 * spt + c2)) / ((mpp + mtt + c1) * (sp + st + c2))
    return full[..., PAD:-PAD, PAD:-PAD].reshape(b, -1).mean(-1)


def to01(x):
    """evaluation/metrics.py:18-19 on an f32 tensor."""
    return x.add(1).mul(0.5)


def _smooth(shape, g):
    b, c, h, w = shape
    low = torch.rand(b, c, max(h // 8, 2) + 2, max(w // 8, 2) + 2, generator=g)
    return F.interpolate(low, size=(h, w), mode="bicubic", align_corners=False).clamp(0, 1)


def cases(shape, seed=0):
    """-> [(name, a, b)]: f32 [B, C, H, W] pairs in [0, 1]: a smooth image against itself plus noise, two independent images, an image
    against its negative (about -0.65), zeros against ones (9.999e-5), and the two flat near-identical pairs on which f32 moments lose the most."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * shape[2] + shape[3] + shape[0])
    smooth = _smooth(shape, g)
    u1, u2 = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    return [
        ("smooth+noise", smooth, (smooth + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)),
        ("independent", u1, u2),
        ("negative", smooth, 1 - smooth),
        ("zeros-ones", torch.zeros(shape), torch.ones(shape)),
        ("flat+1e-3", torch.full(shape, 0.7), 0.7 + 1e-3 * torch.randn(shape, generator=g)),
        ("ones-1e-4", torch.ones(shape), 1 - 1e-4 * torch.rand(shape, generator=g)),
    ]


def pm1(x01):
    """An image on [-1, 1] whose f32 map back, `to01`, is what the kernel's from_pm1 form and the witness are both fed (it is NOT x01 bit for bit)."""
    return x01 * 2 - 1
