"""The GroupNorm kernels on the BatchNorm route (models/patchgan.py: one "image" of N*H*W pixels, groups = C, inv_count) and per-group sensitivity at
groups = 32, each entry point against a float64 evaluation of the same operation on the SAME bf16 / f32 operands (-m gpu).

Inputs: every channel has its own mean in U(-3, 3) and std in U(0.2, 2) before the bf16 rounding, so statistics taken from a neighbouring channel or
group move every output of that channel; gamma ~ 1 + 0.5 N(0, 1), beta ~ 0.3 N(0, 1), da ~ bf16 N(0, 1).  For LeakyReLU (act 2) da is zeroed where the
float64 pre-activation has |u| < 1e-3 (the side of zero is not decidable in f32 there; with da = 0 the element adds nothing to any sum and its dx does
not depend on the slope); the zeroed share is asserted below 0.5 %.

Bars (none is taken from what the kernels give; an f32 evaluation of the kernels' formulas stays inside all of them):
  statistics          |got - ref| <= 1e-5 |ref| per element (f32 partial sums, f64 combine, one f32 rounding); constant input: rstd = 1/sqrt(eps) to 1e-6
  bf16 outputs y, dx  |got - ref| <= 2^-8 |ref| + 1e-5 max|ref| per element (one bf16 rounding plus under ten f32 operations)
  dgamma, dbeta, sums rel_err < 1e-5
  running estimates   1e-6 per element of the f32 blend (see test_batchnorm_running_update)
  activation backward bit-equal

Worst figures observed on an MI355X (bar in brackets; "x bar" = the largest |err| / tolerance over all elements, cases and activations):
  groupnorm_stats                 mean 1.2e-06, rstd 7.0e-07 relative [1e-5]; constant input rstd 4.2e-08 [1e-6]
  groupnorm_apply                 y 0.987 x bar [1]
  groupnorm_bwd_reduce            sums 4.2e-07, dgamma 3.6e-07, dbeta 1.8e-07 rel_err [1e-5]
  groupnorm_bwd_apply (split)     dx 0.990 x bar [1]
  groupnorm_bwd (fused)           dx 0.990 x bar [1]; dgamma 3.6e-07, dbeta 1.8e-07 rel_err [1e-5]
  constant statistics (eval)      y 0.983, dx 0.983 x bar [1]; dgamma 3.1e-07, dbeta 1.8e-07 rel_err [1e-5]
  batchnorm_running_update        running_var 1.6e-07 relative [1e-6], running_mean 1.1e-07 of its terms' magnitude [1e-6];
                                  constant channel: 0.0e+00 from running_var = 0 [m unbias 1e-6 eps = 1e-12 .. 4e-12], 9.1e-08 from a random one [the same + 2^-23 |result|]
  _bn_stats                       running_mean 6.66e-08, running_var 5.68e-08 elem_err [1e-5]; mean 5.2e-08, rstd 2.0e-07 relative [1e-5]
  leaky_relu_bwd / relu_bwd       bit-equal
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import elem_err, rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SLOPE = float(np.float32(0.2))          # the kernels' 0.2f

# (n, hw, c, groups, eps): x is [n, hw, c]
BN_CASES = [(1, 97, 64, 64, 1e-5),          # one ragged chunk
            (1, 2883, 512, 512, 1e-5),      # 3 x 31 x 31, the 512-channel layer; C > 256: two rounds in the block reduce
            (1, 8192, 128, 128, 1e-5),      # several chunks
            (1, 1025, 72, 72, 1e-5)]        # nine live channel lanes of sixteen
GN_CASES = [(2, 16 * 16, 128, 32, 1e-6), (3, 5 * 7, 96, 32, 1e-6)]
CASES = BN_CASES + GN_CASES
ACTS = [0, 1, 2]


def _ops():
    from dmvae_amd import ops
    return ops


def _f32(v):
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def _inputs(n, hw, c):
    """CPU operands exactly as the kernels receive them (bf16 activations, f32 parameters); shared by every test of a shape and never written to."""
    g = torch.Generator().manual_seed(7919 * n + 31 * hw + c)
    mu = torch.rand(c, generator=g) * 6 - 3
    sd = torch.rand(c, generator=g) * 1.8 + 0.2
    x = (torch.randn(n, hw, c, generator=g) * sd + mu).to(BF)
    gamma = 1 + 0.5 * torch.randn(c, generator=g)
    beta = 0.3 * torch.randn(c, generator=g)
    da = torch.randn(n, hw, c, generator=g).to(BF)
    dres = torch.randn(n, hw, c, generator=g).to(BF)
    return x, gamma, beta, da, dres


def _act(u, act):
    return u if act == 0 else (R.swish(u) if act == 1 else F.leaky_relu(u, SLOPE))


def _dact(u, act):
    if act == 0:
        return torch.ones_like(u)
    if act == 1:
        sg = torch.sigmoid(u)
        return sg * (1 + u * (1 - sg))
    return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, SLOPE))


def _norm64(x, gamma, beta, groups, eps):
    """Pre-activation u [n, hw, c] in float64: R.batch_norm in training mode where every channel is its own group of one image, R.group_norm otherwise."""
    n, hw, c = x.shape
    xc = x.permute(0, 2, 1)
    if groups == c and n == 1:
        u, _, _ = R.batch_norm(xc.unsqueeze(-1), gamma, beta, torch.zeros(c, dtype=x.dtype), torch.ones(c, dtype=x.dtype), True, eps=eps)
        u = u.squeeze(-1)
    else:
        u = R.group_norm(xc, gamma, beta, groups, eps)
    return u.permute(0, 2, 1)


def _mask_da(da, u, act):
    """da with the elements whose LeakyReLU side is ambiguous in f32 zeroed (act 2 only) and the zeroed share."""
    if act != 2:
        return da, 0.0
    amb = u.abs() < 1e-3
    return da.masked_fill(amb, 0), amb.double().mean().item()


@functools.lru_cache(maxsize=None)
def _ref(n, hw, c, groups, eps, act):
    x, gamma, beta, da, _ = _inputs(n, hw, c)
    eps = _f32(eps)
    x64, g64, b64 = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    u = _norm64(x64, g64, b64, groups, eps)
    ud = u.detach()
    da_used, share = _mask_da(da, ud, act)
    y = _act(u, act)
    y.backward(da_used.double())
    cpg = c // groups
    xg = x64.detach().permute(0, 2, 1).reshape(n, groups, -1)
    mean, rstd = xg.mean(-1), 1 / torch.sqrt(xg.var(-1, unbiased=False) + eps)
    xh = (x64.detach() - mean.repeat_interleave(cpg, 1)[:, None, :]) * rstd.repeat_interleave(cpg, 1)[:, None, :]
    gd = da_used.double() * _dact(ud, act) * g64.detach()
    sums = torch.stack([gd.sum(1).reshape(n, groups, cpg).sum(-1), (gd * xh).sum(1).reshape(n, groups, cpg).sum(-1)], -1)
    return dict(y=y.detach(), dx=x64.grad, dg=g64.grad, db=b64.grad, sums=sums, mean=mean, rstd=rstd, da=da_used, share=share)


def _dev(n, hw, c):
    x, gamma, beta, da, dres = _inputs(n, hw, c)
    return x.to(DEV), gamma.to(DEV), beta.to(DEV), da.to(DEV), dres.to(DEV)


def _rel_each(got, ref, bar, what):
    got, ref = got.detach().cpu().double(), ref.double()
    e = ((got - ref).abs() / ref.abs()).max().item()
    print(f"[fig] {what}: max relative error {e:.2e} (bar {bar:.0e})")
    assert e <= bar, (what, e)


def _bf16_bar(got, ref, what):
    got, ref = got.detach().float().cpu().double(), ref.double()
    tol = 2.0 ** -8 * ref.abs() + 1e-5 * ref.abs().max()
    e = ((got - ref).abs() / tol).max().item()
    print(f"[fig] {what}: worst |err| / (2^-8 |ref| + 1e-5 max|ref|) = {e:.3f} (bar 1)")
    assert e <= 1.0, (what, e)


def _rel_bar(got, ref, what, bar=1e-5):
    e = rel_err(got.detach().cpu(), ref)
    print(f"[fig] {what}: rel_err {e:.2e} (bar {bar:.0e})")
    assert e < bar, (what, e)


@pytest.mark.parametrize("case", CASES)
def test_groupnorm_stats(case):
    n, hw, c, groups, eps = case
    x = _dev(n, hw, c)[0]
    st = _ops().groupnorm_stats(x, groups=groups, eps=eps)
    r = _ref(*case, 0)
    assert st.shape == (n, groups, 2)
    _rel_each(st[..., 0], r["mean"], 1e-5, f"stats mean {case}")
    _rel_each(st[..., 1], r["rstd"], 1e-5, f"stats rstd {case}")
    assert torch.equal(_ops().groupnorm_stats(x, groups=groups, eps=eps), st)


@pytest.mark.parametrize("case", [(1, 1025, 72, 72, 1e-5), (1, 2883, 512, 512, 1e-5), (2, 16 * 16, 128, 32, 1e-6)])
def test_groupnorm_stats_constant_input(case):
    """Zero variance: the f32 sums of 3.0 and 9.0 are exact, so the variance is exactly 0 and rstd = 1/sqrt(eps) (no negative variance, no NaN)."""
    n, hw, c, groups, eps = case
    st = _ops().groupnorm_stats(torch.full((n, hw, c), 3.0, dtype=BF, device=DEV), groups=groups, eps=eps).cpu().double()
    want = 1 / np.sqrt(_f32(eps))
    e = ((st[..., 1] - want).abs() / want).max().item()
    print(f"[fig] constant input rstd {case}: max relative error {e:.2e} (bar 1e-6)")
    assert (st[..., 0] == 3.0).all() and e <= 1e-6


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", CASES)
def test_groupnorm_apply(case, act):
    n, hw, c, groups, eps = case
    ops = _ops()
    x, gamma, beta, _, _ = _dev(n, hw, c)
    st = ops.groupnorm_stats(x, groups=groups, eps=eps)
    y = ops.groupnorm_apply(x, st, gamma, beta, act, groups=groups)
    assert y.dtype == BF and y.shape == x.shape
    _bf16_bar(y, _ref(*case, act)["y"], f"apply y {case} act {act}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", CASES)
def test_groupnorm_bwd_reduce_then_apply(case, act):
    n, hw, c, groups, eps = case
    ops = _ops()
    r = _ref(*case, act)
    assert r["share"] < 5e-3, r["share"]
    x, gamma, beta, _, _ = _dev(n, hw, c)
    da = r["da"].to(DEV)
    st = ops.groupnorm_stats(x, groups=groups, eps=eps)
    sums, dg, db = ops.groupnorm_bwd_reduce(da, x, st, gamma, beta, act, groups=groups)
    assert sums.shape == (n, groups, 2)
    _rel_bar(sums, r["sums"], f"reduce sums {case} act {act}")
    _rel_bar(dg, r["dg"], f"reduce dgamma {case} act {act}")
    _rel_bar(db, r["db"], f"reduce dbeta {case} act {act}")
    dx = ops.groupnorm_bwd_apply(da, x, st, sums, gamma, beta, act, groups=groups, inv_count=1.0 / ((c // groups) * hw))
    _bf16_bar(dx, r["dx"], f"split dx {case} act {act}")


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_groupnorm_bwd_fused(case, act, with_dres):
    n, hw, c, groups, eps = case
    ops = _ops()
    r = _ref(*case, act)
    x, gamma, beta, da, dres = _dev(n, hw, c)
    st = ops.groupnorm_stats(x, groups=groups, eps=eps)
    dx, dg, db = ops.groupnorm_bwd(da, x, st, gamma, beta, bool(act), dres=dres if with_dres else None, groups=groups)
    want = r["dx"] + _inputs(n, hw, c)[4].double() if with_dres else r["dx"]
    _bf16_bar(dx, want, f"fused dx {case} act {act} dres {with_dres}")
    _rel_bar(dg, r["dg"], f"fused dgamma {case} act {act}")
    _rel_bar(db, r["db"], f"fused dbeta {case} act {act}")


@pytest.mark.parametrize("case", [(1, 2883, 512, 512, 1e-5), (1, 1025, 72, 72, 1e-5), (3, 5 * 7, 96, 32, 1e-6)])
def test_inv_count(case):
    """inv_count <= 0 is 1 / (channels per group * hw); two ranks holding the same batch (sums doubled by the all-reduce, inv_count halved) give one
    rank's bits: the factor 2 moves between the two operands of one f32 product."""
    n, hw, c, groups, eps = case
    ops = _ops()
    x, gamma, beta, da, _ = _dev(n, hw, c)
    st = ops.groupnorm_stats(x, groups=groups, eps=eps)
    inv = 1.0 / ((c // groups) * hw)
    for act in ACTS:
        sums, _, _ = ops.groupnorm_bwd_reduce(da, x, st, gamma, beta, act, groups=groups, need_param_grads=False)
        one = ops.groupnorm_bwd_apply(da, x, st, sums, gamma, beta, act, groups=groups, inv_count=inv)
        assert torch.equal(ops.groupnorm_bwd_apply(da, x, st, sums, gamma, beta, act, groups=groups, inv_count=0.0), one)
        assert torch.equal(ops.groupnorm_bwd_apply(da, x, st, sums, gamma, beta, act, groups=groups, inv_count=-1.0), one)
        assert torch.equal(ops.groupnorm_bwd_apply(da, x, st, 2 * sums, gamma, beta, act, groups=groups, inv_count=0.5 * inv), one)
        # and the count is really used: another one changes dx
        assert not torch.equal(ops.groupnorm_bwd_apply(da, x, st, sums, gamma, beta, act, groups=groups, inv_count=2 * inv), one)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", [(1, 2883, 512, 512, 1e-5), (1, 1025, 72, 72, 1e-5)])
def test_constant_statistics_eval_mode(case, act):
    """An eval-mode BatchNorm: `stats` are the running estimates, constants that are NOT the batch's, and sums = 0.  Then dx = rstd gamma da act'(u),
    dgamma = sum da act'(u) x_hat and dbeta = sum da act'(u), all with the given statistics."""
    n, hw, c, groups, eps = case
    ops = _ops()
    x, gamma, beta, da, _ = _inputs(n, hw, c)
    g = torch.Generator().manual_seed(c + act)
    mean = x.float().mean(dim=(0, 1)) + torch.rand(c, generator=g) - 0.5
    rstd = torch.rand(c, generator=g) * 2.7 + 0.3
    st = torch.stack([mean, rstd], dim=1).view(1, c, 2).contiguous()
    xh = (x.double() - mean.double()) * rstd.double()
    u = xh * gamma.double() + beta.double()
    da, share = _mask_da(da, u, act)
    assert share < 5e-3, share
    dy = da.double() * _dact(u, act)
    xd, gd, bd, dad, std = x.to(DEV), gamma.to(DEV), beta.to(DEV), da.to(DEV), st.to(DEV)
    _bf16_bar(ops.groupnorm_apply(xd, std, gd, bd, act, groups=c), _act(u, act), f"eval y {case} act {act}")
    dx = ops.groupnorm_bwd_apply(dad, xd, std, torch.zeros(1, c, 2, device=DEV), gd, bd, act, groups=c, inv_count=1.0 / hw)
    _bf16_bar(dx, rstd.double() * gamma.double() * dy, f"eval dx {case} act {act}")
    _, dg, db = ops.groupnorm_bwd_reduce(dad, xd, std, gd, bd, act, groups=c)
    _rel_bar(dg, (dy * xh).sum(dim=(0, 1)), f"eval dgamma {case} act {act}")
    _rel_bar(db, dy.sum(dim=(0, 1)), f"eval dbeta {case} act {act}")


@pytest.mark.parametrize("case", [(1, 1025, 72, 72, 1e-5), (2, 16 * 16, 128, 32, 1e-6)])
def test_output_buffers(case):
    n, hw, c, groups, eps = case
    ops = _ops()
    x, gamma, beta, da, _ = _dev(n, hw, c)
    st = ops.groupnorm_stats(x, groups=groups, eps=eps)
    sums, dg, db = ops.groupnorm_bwd_reduce(da, x, st, gamma, beta, 2, groups=groups)
    dg_out, db_out = torch.full((c,), float("nan"), device=DEV), torch.full((c,), float("nan"), device=DEV)
    sums2, dg2, db2 = ops.groupnorm_bwd_reduce(da, x, st, gamma, beta, 2, groups=groups, dg_out=dg_out, db_out=db_out)
    assert dg2 is dg_out and db2 is db_out and torch.equal(dg_out, dg) and torch.equal(db_out, db) and torch.equal(sums2, sums)
    sums3, dg3, db3 = ops.groupnorm_bwd_reduce(da, x, st, gamma, beta, 2, groups=groups, need_param_grads=False)
    assert dg3 is None and db3 is None and torch.equal(sums3, sums)
    # the fused entry: the same contract, and dx does not depend on whether the parameter gradients ride along
    dx, dgf, dbf = ops.groupnorm_bwd(da, x, st, gamma, beta, True, groups=groups)
    dg_out.fill_(float("nan")), db_out.fill_(float("nan"))
    dx2, dg4, db4 = ops.groupnorm_bwd(da, x, st, gamma, beta, True, groups=groups, dg_out=dg_out, db_out=db_out)
    assert dg4 is dg_out and db4 is db_out and torch.equal(dg_out, dgf) and torch.equal(db_out, dbf) and torch.equal(dx2, dx)
    dx3, dg5, db5 = ops.groupnorm_bwd(da, x, st, gamma, beta, True, groups=groups, need_param_grads=False)
    assert dg5 is None and db5 is None and torch.equal(dx3, dx)


@pytest.mark.parametrize("n_count", [72, 8192])
@pytest.mark.parametrize("momentum", [0.1, 0.37])
def test_batchnorm_running_update(momentum, n_count):
    """running_mean' = (1 - m) running_mean + m mean; running_var' = (1 - m) running_var + m unbias max(1 / rstd^2 - eps, 0), against float64 on the f32
    operands and f32-rounded scalars.  The kernel makes five f32 roundings on the way to running_var' (rstd^2, the reciprocal, - eps, x unbias x m, the
    blend), all of its terms positive with var >= 1e-2 >> eps: 1e-6 relative per element.  running_mean' may cancel, so its 1e-6 is relative to the
    magnitude of the two terms that are added."""
    ops = _ops()
    c, eps = 300, 1e-5                                             # two blocks of 256 threads
    unbias = n_count / (n_count - 1)
    g = torch.Generator().manual_seed(n_count + int(100 * momentum))
    mean = torch.rand(c, generator=g) * 6 - 3
    var = torch.rand(c, generator=g) * 4 + 1e-2
    rstd = (1 / torch.sqrt(var.double() + eps)).float()
    rstd[7] = _f32(1 / np.sqrt(_f32(eps)))                         # what groupnorm_stats gives for a constant channel
    rstd[8] = rstd[7]
    rm0 = torch.randn(c, generator=g)
    rv0 = torch.rand(c, generator=g) * 3 + 0.05
    rv0[8] = 0.0
    st = torch.stack([mean, rstd], dim=1).view(1, c, 2).contiguous()
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    ops.batchnorm_running_update(st.to(DEV), rm, rv, eps, momentum, unbias)
    m, ub, e = _f32(momentum), _f32(unbias), _f32(eps)
    var64 = (1 / rstd.double() ** 2 - e).clamp_min(0)
    rm_ref = (1 - m) * rm0.double() + m * mean.double()
    rv_ref = (1 - m) * rv0.double() + m * ub * var64
    live = torch.ones(c, dtype=torch.bool)
    live[7] = live[8] = False
    assert (var64[live] >= 1e-2).all()
    e_rv = ((rv.cpu().double() - rv_ref).abs() / rv_ref)[live].max().item()
    e_rm = ((rm.cpu().double() - rm_ref).abs() / ((1 - m) * rm0.double().abs() + m * mean.double().abs())).max().item()
    print(f"[fig] running_var m {momentum} n {n_count}: max relative error {e_rv:.2e} (bar 1e-6); running_mean {e_rm:.2e} of the terms' magnitude (bar 1e-6)")
    assert e_rv <= 1e-6 and e_rm <= 1e-6
    # a constant channel (rstd = 1/sqrt(eps)): its variance is 0 up to the roundings of rstd^2 and the reciprocal, i.e. below 1e-6 eps.  Channel 8 starts from
    # running_var = 0, so nothing else is in the result; channel 7 starts from a random one, whose blend adds the roundings of an f32 product and sum
    # (2^-23 of the result) on top.
    bound = m * ub * 1e-6 * e
    d8, d7 = abs(rv[8].item() - 0.0), abs(rv[7].item() - (1 - m) * rv0[7].double().item())
    print(f"[fig] constant channel m {momentum} n {n_count}: |running_var' - (1 - m) running_var| = {d8:.2e} from 0, {d7:.2e} from {rv0[7].item():.3f} (bar {bound:.2e}, + 2^-23 |result| for the latter)")
    assert d8 <= bound and d7 <= bound + 2.0 ** -23 * rv[7].item()


def test_bn_stats_updates_the_running_estimates():
    """models/patchgan.py::_bn_stats on an nn.BatchNorm2d in training mode: one call leaves nn.BatchNorm2d's running estimates (momentum 0.1, unbiased
    variance) of the same bf16 input and counts one batch."""
    from dmvae_amd.models.patchgan import _bn_stats
    b, h, w_, c = 2, 9, 11, 72
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(b, h, w_, c, generator=g) * (torch.rand(c, generator=g) * 1.8 + 0.2) + (torch.rand(c, generator=g) * 6 - 3)).to(BF)
    bn = torch.nn.BatchNorm2d(c)
    rm0, rv0 = torch.randn(c, generator=g), torch.rand(c, generator=g) * 3 + 0.05
    with torch.no_grad():
        bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
    bn = bn.to(DEV).train()
    st, batch_stats, count, group = _bn_stats(bn, x.to(DEV))
    x64 = x.double().permute(0, 3, 1, 2)
    _, rm_ref, rv_ref = R.batch_norm(x64, torch.ones(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64), rm0.double(), rv0.double(), True,
                                     momentum=0.1, eps=1e-5)
    e_rm, e_rv = elem_err(bn.running_mean.cpu(), rm_ref), elem_err(bn.running_var.cpu(), rv_ref)
    print(f"[fig] _bn_stats running_mean elem_err {e_rm:.2e}, running_var elem_err {e_rv:.2e} (bar 1e-5)")
    assert batch_stats and count == b * h * w_ and group is None and st.shape == (1, c, 2)
    assert e_rm < 1e-5 and e_rv < 1e-5
    assert bn.num_batches_tracked.item() == 1
    _rel_each(st[0, :, 0], x64.mean(dim=(0, 2, 3)), 1e-5, "_bn_stats mean")
    _rel_each(st[0, :, 1], 1 / torch.sqrt(x64.var(dim=(0, 2, 3), unbiased=False) + _f32(1e-5)), 1e-5, "_bn_stats rstd")
    # eval mode: the running estimates as constants, nothing updated
    bn.eval()
    rm1, rv1 = bn.running_mean.clone(), bn.running_var.clone()
    st2, batch_stats2, _, _ = _bn_stats(bn, x.to(DEV))
    assert not batch_stats2 and torch.equal(bn.running_mean, rm1) and torch.equal(bn.running_var, rv1) and bn.num_batches_tracked.item() == 1
    assert torch.equal(st2[0, :, 0], rm1)
    _rel_each(st2[0, :, 1], 1 / torch.sqrt(rv1.cpu().double() + _f32(1e-5)), 1e-6, "_bn_stats eval rstd")


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("n", [8, 8 * 1000 + 8])
def test_leaky_relu_and_relu_bwd_bit_exact(n):
    """dx = y > 0 ? dy : bf16(slope * dy), bit for bit (the sign of a zero included), with y = 0 and y = -0.0 entries: both are "not positive"."""
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    y = torch.randn(n, generator=g).to(BF)
    dy = torch.randn(n, generator=g).to(BF)
    y[0], y[1], y[n - 1], y[n - 2] = 0.0, -0.0, 0.0, -0.0
    dy[2], dy[3] = 0.0, -0.0
    for slope, fn in ((SLOPE, lambda a, b: ops.leaky_relu_bwd(a, b)), (0.5, lambda a, b: ops.leaky_relu_bwd(a, b, slope=0.5)), (0.0, ops.relu_bwd)):
        want = torch.where(y.float() > 0, dy, (dy.float() * torch.tensor(slope, dtype=torch.float32)).to(BF))     # an f32 product, one bf16 rounding
        got = fn(dy.to(DEV), y.to(DEV)).cpu()
        assert torch.equal(_bits(got), _bits(want)), slope
