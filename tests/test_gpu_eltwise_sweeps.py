"""One case past the grid cap for every elementwise / layout launcher that goes through grid_for(..., 256, 4096) (-m gpu): 4096 blocks x 256 threads x 8
elements = 8,388,608 elements per sweep of the grid-stride loop, where every other test of these kernels stays inside the first sweep and decoder
activations have 268 M elements.  Index ops are held bit-exact against torch indexing, arithmetic ones against float64 on the same bf16 operands:
|got - ref| <= 2^-8 |ref| + 1e-5 max|ref| per element (one bf16 rounding plus under ten f32 operations); col2im at its existing 4e-3 relative-to-max.

Every output is allocated with a guard region behind it (the wrappers' torch.empty / torch.empty_like are replaced by a guarded allocator for the call):
the guard must come back untouched, and the last eight elements of every output are checked on their own.

Worst figures observed on an MI355X (bar in brackets; "x bar" = the largest |err| / tolerance over all elements, then over the last eight):
  silu       0.885, 0.864 x bar [1]
  silu_bwd   0.988, 0.369 x bar [1]
  gelu_bwd   0.987, 0.762 x bar [1]
  col2im     rel_err 2.9e-03, last eight 0.0e+00 [4e-3]
  relu_bwd, leaky_relu_bwd, sumpool2x2, maxpool2x2, maxpool2x2_relu_bwd, nchw_to_nhwc_bf16 (both kernels), nhwc_to_nchw_f32 (both source types), im2col: bit-equal
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SWEEP = 4096 * 256 * 8                       # elements one sweep of an 8-wide grid_for(..., 256, 4096) launch covers
N_ELT = SWEEP + 8 * 777
POOL_OUT = (3, 95, 121, 248)                 # 8,551,560 elements > SWEEP; 31 channel octets; its 2x2 source has 34.2 M elements (68 MB)
GUARD, FILL = 4096, 0xA5


def _ops():
    from dmvae_amd import ops
    return ops


class _GuardedTorch:
    """Stands in for the `torch` name inside dmvae_amd.ops: empty / empty_like hand out the front of a larger buffer pre-filled with a byte pattern, so that
    an element the kernel does not write and a write past the end both show; everything else is torch's."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=None, device=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
        self.bufs.append((raw, nbytes))
        return raw[:nbytes].view(dtype).view(shape)

    def empty_like(self, t):
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)

    def check(self):
        assert self.bufs, "the wrapper allocated nothing through torch.empty / torch.empty_like"
        for raw, nbytes in self.bufs:
            assert (raw[nbytes:] == FILL).all(), "a write landed behind the end of an output"


@pytest.fixture
def guarded(monkeypatch):
    ops = _ops()
    g = _GuardedTorch()
    monkeypatch.setattr(ops, "torch", g)
    yield g
    g.check()


@pytest.fixture(scope="module")
def base():
    """34.2 M bf16 N(0, 1) values from a seeded CPU generator, on the GPU; every test takes its operands from it (read only)."""
    n, h, w_, c = POOL_OUT
    gen = torch.Generator().manual_seed(41)
    t = torch.randn(n * 2 * h * 2 * w_ * c, generator=gen).to(BF).to(DEV)
    yield t
    del t


def _take(base, shape, offset=0):
    """A view of `base`; offsets are multiples of 8 elements: the kernels read 16 bytes at a time."""
    assert offset % 8 == 0
    k = math.prod(shape)
    return base[offset:offset + k].view(shape)


def _bf16_bar(got, ref, what):
    got, ref = got.float().cpu().double().flatten(), ref.double().flatten()
    scale = 1e-5 * ref.abs().max()
    ratio = (got - ref).abs() / (2.0 ** -8 * ref.abs() + scale)
    e, e8 = ratio.max().item(), ratio[-8:].max().item()
    print(f"[fig] {what}: worst |err| / (2^-8 |ref| + 1e-5 max|ref|) = {e:.3f}, last eight {e8:.3f} (bar 1)")
    assert e <= 1.0 and e8 <= 1.0, (what, e)


def _same(got, want, what):
    """Bit-exact index ops: the values are equal everywhere (the last eight elements on their own, so that a failure names the tail)."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert torch.equal(got.flatten()[-8:], want.flatten()[-8:]), what + ": last eight elements"
    assert torch.equal(got, want), what


# ---- arithmetic: silu, silu_bwd, gelu_bwd --------------------------------------------------------------------------------------------------------------
def test_silu_fwd_bwd_past_the_cap(base, guarded):
    ops = _ops()
    x, dy = _take(base, (N_ELT,)) * 3, _take(base, (N_ELT,), N_ELT)         # x ~ N(0, 3^2) (still bf16: a product of bf16 values is rounded back by torch)
    y, dx = ops.silu(x), ops.silu_bwd(x, dy)
    xr = x.float().cpu().double().requires_grad_(True)
    yr = F.silu(xr)
    yr.backward(dy.float().cpu().double())
    _bf16_bar(y, yr.detach(), "silu")
    _bf16_bar(dx, xr.grad, "silu_bwd")


def test_gelu_bwd_past_the_cap(base, guarded):
    ops = _ops()
    x, dy = _take(base, (N_ELT,), 3 * N_ELT) * 2, _take(base, (N_ELT,), 2 * N_ELT)
    dx = ops.gelu_bwd(dy, x)
    xr = x.float().cpu().double().requires_grad_(True)
    F.gelu(xr).backward(dy.float().cpu().double())
    _bf16_bar(dx, xr.grad, "gelu_bwd")


# ---- bit-exact --------------------------------------------------------------------------------------------------------------------------------------------------
def test_relu_and_leaky_relu_bwd_past_the_cap(base, guarded):
    ops = _ops()
    y, dy = _take(base, (N_ELT,), 8), _take(base, (N_ELT,), N_ELT + 24)
    slope = torch.tensor(0.2, dtype=torch.float32, device=DEV)
    _same(ops.relu_bwd(dy, y), torch.where(y.float() > 0, dy, torch.zeros_like(dy)), "relu_bwd")
    _same(ops.leaky_relu_bwd(dy, y), torch.where(y.float() > 0, dy, (dy.float() * slope).to(BF)), "leaky_relu_bwd")


def _windows(x):
    """The four members of every 2x2 window of x [n, 2h, 2w, c] in scan order, each [n, h, w, c]."""
    n, h2, w2, c = x.shape
    v = x.view(n, h2 // 2, 2, w2 // 2, 2, c)
    return [v[:, :, k >> 1, :, k & 1, :] for k in range(4)]


def _first_max(v):
    m, arg = v[0].float(), torch.zeros(v[0].shape, dtype=torch.int8, device=v[0].device)
    for k in range(1, 4):
        gt = v[k].float() > m
        arg = torch.where(gt, torch.full_like(arg, k), arg)
        m = torch.where(gt, v[k].float(), m)
    return m, arg


def test_sumpool_and_maxpool_past_the_cap(base, guarded):
    ops = _ops()
    n, h, w_, c = POOL_OUT
    x = _take(base, (n, 2 * h, 2 * w_, c))
    v = _windows(x)
    want = (((v[0].float() + v[1].float()) + v[2].float()) + v[3].float()).to(BF)      # the kernel's order of f32 additions, one bf16 rounding
    _same(ops.sumpool2x2(x), want, "sumpool2x2")
    _same(ops.maxpool2x2(x), _first_max(v)[0].to(BF), "maxpool2x2")


def test_maxpool_relu_bwd_past_the_cap(base, guarded):
    ops = _ops()
    n, h, w_, c = POOL_OUT
    x = _take(base, (n, 2 * h, 2 * w_, c))
    extra = base.roll(12345).view(x.shape)
    dpool = -_take(base, POOL_OUT, 776)
    dx = ops.maxpool2x2_relu_bwd(dpool, x, extra)
    v = _windows(x)
    _, arg = _first_max(v)
    want = torch.empty_like(x)
    wv = want.view(n, h, 2, w_, 2, c)
    ev = _windows(extra)
    for k in range(4):
        t = (torch.where(arg == k, dpool.float(), torch.zeros((), device=DEV)) + ev[k].float()).to(BF)
        wv[:, :, k >> 1, :, k & 1, :] = torch.where(v[k].float() > 0, t, torch.zeros_like(t))
    _same(dx, want, "maxpool2x2_relu_bwd")
    assert (arg > 0).any() and (dx == 0).any()


def test_layout_ops_past_the_cap(base, guarded):
    ops = _ops()
    n, c, h, w_ = 3, 3, 600, 590                                # 1,062,000 pixels > 1,048,576: one pixel (octet) per thread
    x = _take(base, (n, c, h, w_)).float() * 1.37               # f32 values that are not bf16 values
    nhwc = ops.nchw_to_nhwc_bf16(x, c_pad=8)
    want = torch.zeros(n, h, w_, 8, dtype=BF, device=DEV)
    want[..., :c] = x.permute(0, 2, 3, 1).to(BF)
    _same(nhwc, want, "nchw_to_nhwc_bf16 c_pad 8")
    _same(ops.nchw_to_nhwc_bf16(x), x.permute(0, 2, 3, 1).to(BF).contiguous(), "nchw_to_nhwc_bf16 unpadded (the scalar kernel)")
    src = _take(base, (n, h, w_, 8), 96)
    _same(ops.nhwc_to_nchw_f32(src, c), src[..., :c].permute(0, 3, 1, 2).float().contiguous(), "nhwc_to_nchw_f32 from bf16")
    _same(ops.nhwc_to_nchw_f32(src.float(), c), src[..., :c].permute(0, 3, 1, 2).float().contiguous(), "nhwc_to_nchw_f32 from f32")


def test_im2col_past_the_cap(base, guarded):
    ops = _ops()
    n, h, w_, c = 3, 102, 98, 72                                # 3 x 51 x 49 x 16 taps x 9 octets = 1,079,568 threads' worth
    x = _take(base, (n, h, w_, c), 32)
    col = ops.im2col(x, 4, 2, 1)
    ho, wo = h // 2, w_ // 2
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    want = torch.cat([xp[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2, :] for ky in range(4) for kx in range(4)], dim=-1)
    _same(col, want.contiguous(), "im2col k4 s2 p1")


def test_col2im_past_the_cap(base, guarded):
    ops = _ops()
    n, h, w_, c = 3, 190, 186, 80                               # 8,481,600 output elements > SWEEP; the columns are 33.9 M (68 MB)
    ho, wo = h // 2, w_ // 2
    dcol = _take(base, (n, ho, wo, 16 * c))
    dx = ops.col2im(dcol, h, w_, 4, 2, 1)
    ref = torch.zeros(n, h + 2, w_ + 2, c, dtype=torch.float64, device=DEV)
    for ky in range(4):
        for kx in range(4):
            t = ky * 4 + kx
            ref[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2, :] += dcol[..., t * c:(t + 1) * c].double()
    ref = ref[:, 1:h + 1, 1:w_ + 1, :].cpu()
    got = dx.float().cpu()
    e, e8 = rel_err(got, ref), ((got.flatten()[-8:].double() - ref.flatten()[-8:]).abs().max() / ref.abs().max()).item()
    print(f"[fig] col2im k4 s2 p1: rel_err {e:.2e}, last eight {e8:.2e} (bar 4e-3)")
    assert e < 4e-3 and e8 < 4e-3
