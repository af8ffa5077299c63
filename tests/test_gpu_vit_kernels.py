"""The ViT encoder's row kernels (csrc/vit.hip, csrc/vit_bwd.hip) through their ops wrappers, every width and thread layout, against the fp64 definitions and
element-wise bars of tests/vit_kernels_spec.py (-m gpu).  The references run on the GPU in torch double.  Wrapper-allocated outputs come from the guarded
allocator of tests/test_gpu_eltwise_sweeps.py, pre-filled with NaN; caller-allocated in-place tensors are views into a sentinel-filled buffer with a guard on
both sides.  Every case asserts that a second call gives the same bits.

Which instantiation a case launches:
  layernorm_bf16               layernorm_kernel<C / 256, false, C == 384>          at all seven widths; rows 1, 3, 5: idle waves in the last block
  scale_residual_layernorm_    layernorm_kernel<C / 256, true, C == 384>           the same
  layernorm_bwd_               layernorm_bwd_kernel<C / 256, C == 384>             at all seven widths; 1027 and 2500 rows: second and ragged third round of the 1024 waves
  layerscale_bwd               c / 8 lanes x 256 / (c / 8) rows: 8 -> 1 x 256, 256 -> 32 x 8, 384 -> 48 x 5 (16 idle), 512 -> 64 x 4, 768 -> 96 x 2 (64 idle),
                               1024 -> 128 x 2, 1280 -> 160 x 1 (96 idle), 1536 -> 192 x 1 (64 idle), 2048 -> 256 x 1
  layerscale_bwd_dx, scale_residual_, gelu: one case each past the 4096-block grid cap (a second sweep of the grid-stride loop)

Worst figures observed on an MI355X (bar in brackets; |err| / bound over every element of every case):
  layernorm y 0.986, fused 0.986 [1]; the fused form's stream and scale_residual_ 0.990 [1] (one rounding: 2^-24 |ref| * 1.01)
  layernorm_bwd dx 0.050, dgamma 0.136, dbeta 0.143 [1]; layerscale_bwd dgamma 0.220 [1], dy and layerscale_bwd_dx bit-equal
  gelu 0.965, against its approximant 0.965 [1]; gelu_bwd 0.984 [1]; softmax 0.986 [1], row sums within cols * 2^-9 of 1
The bf16 figures are a half-ulp at the bottom of a binade under the factor 1.01, the same ones the f32 CPU emulations give; no test found a kernel at fault.
"""
import pytest
import torch

import vit_kernels_spec as S
from test_gpu_eltwise_sweeps import SWEEP, _GuardedTorch
from vit_kernels_spec import BF, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -768.0          # exact in bf16 and f32; no case produces it
GUARD = 1024           # elements on each side of an in-place tensor


def _ops():
    from dmvae_amd import ops
    return ops


class _NanGuardedTorch(_GuardedTorch):
    """the guarded allocator with the payload pre-filled with NaN (all bits set, in bf16 and f32 alike): an element the kernel leaves unwritten fails its bar"""

    def empty(self, *shape, dtype=None, device=None):
        t = super().empty(*shape, dtype=dtype, device=device)
        raw, nbytes = self.bufs[-1]
        raw[:nbytes].fill_(0xFF)
        return t


@pytest.fixture
def figs():
    """prints the worst |err| / bound of every bar the test went through"""
    S.FIG.clear()
    yield S.FIG
    for k, v in S.FIG.items():
        print("[fig] %s: worst |err| / bound %.3f (bar 1)" % (k, v))


@pytest.fixture
def guarded(monkeypatch, figs):
    ops = _ops()
    g = _NanGuardedTorch()
    monkeypatch.setattr(ops, "torch", g)
    yield g
    torch.cuda.synchronize()
    g.check()


class InPlace:
    """guard | payload | guard in one sentinel-filled buffer; the payload starts as `init`"""

    def __init__(self, init):
        n = init.numel()
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=init.dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(init.shape)
        self.t.copy_(init)

    def ok(self, what):
        assert bool((self.buf[:GUARD] == SENT).all()), what + ": written before the tensor"
        assert bool((self.buf[GUARD + self.t.numel():] == SENT).all()), what + ": written past the tensor"
        return self.t


# ---- LayerNorm forward and the fused LayerScale + residual + LayerNorm ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.LN_WIDTHS)
def test_layernorm_forward_and_fused_form(c, guarded):
    ops = _ops()
    for kind, rows in S.ln_cases(S.LN_FWD_ROWS, S.LN_FWD_HARD):
        k = S.to_dev(S.ln_case(kind, rows, c), DEV)
        what = "%s rows %d width %d" % (kind, rows, c)
        y = ops.layernorm_bf16(k["x"], k["gamma"], k["beta"])
        S.check_layernorm(y, k["x"], k["gamma"], k["beta"], what)
        assert torch.equal(y, ops.layernorm_bf16(k["x"], k["gamma"], k["beta"])), what + ": second call differs"
        # fused against the two kernels, bit for bit: the stream and the tokens
        xa, xb, xc = InPlace(k["x0"]), InPlace(k["x0"]), InPlace(k["x0"])
        ya = ops.scale_residual_layernorm_(xa.t, k["r"], k["ls"], k["gamma"], k["beta"])
        ops.scale_residual_(xb.t, k["r"], k["ls"])
        yb = ops.layernorm_bf16(xb.t, k["gamma"], k["beta"])
        yc = ops.scale_residual_layernorm_(xc.t, k["r"], k["ls"], k["gamma"], k["beta"])
        assert torch.equal(xa.ok(what + " fused"), xb.ok(what + " scale_residual_")), what + ": the fused form's stream differs from scale_residual_'s"
        assert torch.equal(ya, yb), what + ": the fused form's tokens differ from the two kernels'"
        assert torch.equal(xa.t, xc.ok(what)) and torch.equal(ya, yc), what + ": second fused call differs"
        S.check_scale_residual(xa.t, k["x0"], k["r"], k["ls"], what + " stream")
        S.check_layernorm(ya, xa.t, k["gamma"], k["beta"], what + " fused", key="layernorm y (fused)")


# ---- LayerNorm backward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.LN_WIDTHS)
def test_layernorm_backward(c, guarded):
    ops = _ops()
    for kind, rows in S.ln_cases(S.LN_BWD_ROWS, S.LN_BWD_HARD):
        k = S.to_dev(S.ln_case(kind, rows, c), DEV)
        what = "%s rows %d width %d" % (kind, rows, c)
        dx = InPlace(k["dres"])
        dg, db = ops.layernorm_bwd_(dx.t, k["dy"], k["x"], k["gamma"])
        o = S.check_layernorm_bwd(dx.ok(what), dg, db, k["dres"], k["dy"], k["x"], k["gamma"], what)
        dx2 = InPlace(k["dres"])
        dg2, db2 = ops.layernorm_bwd_(dx2.t, k["dy"], k["x"], k["gamma"])
        assert torch.equal(dx.t, dx2.ok(what)) and torch.equal(dg, dg2) and torch.equal(db, db2), what + ": second call differs"
        dx3 = InPlace(k["dres"])
        assert ops.layernorm_bwd_(dx3.t, k["dy"], k["x"], k["gamma"], need_param_grads=False) == (None, None)
        assert torch.equal(dx.t, dx3.ok(what)), what + ": dx without the parameter gradients differs"
        dx4, dgo, dbo = InPlace(k["dres"]), InPlace(k["dg0"]), InPlace(k["db0"])
        r = ops.layernorm_bwd_(dx4.t, k["dy"], k["x"], k["gamma"], dg_out=dgo.t, db_out=dbo.t, accumulate=True)
        assert r[0] is dgo.t and r[1] is dbo.t
        S.check_layernorm_bwd(dx4.ok(what), dgo.ok(what + " dg_out"), dbo.ok(what + " db_out"), k["dres"], k["dy"], k["x"], k["gamma"], what + " accumulate",
                              dg0=k["dg0"], db0=k["db0"], ref=o)
        assert torch.equal(dx.t, dx4.t), what + ": dx of the accumulating call differs"


# ---- LayerScale backward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.LS_WIDTHS)
def test_layerscale_bwd(c, guarded):
    """8 and 2048 are the edges of the argument check (c % 8 == 0, 8 <= c <= 2048); the wrapper takes both."""
    ops = _ops()
    for rows in S.ls_rows(c):
        k = S.to_dev(S.ls_case(rows, c), DEV)
        what = "rows %d width %d" % (rows, c)
        dy, dg = ops.layerscale_bwd(k["dt"], k["y"], k["gamma"])
        S.check_layerscale_bwd(dy, dg, k["dt"], k["y"], k["gamma"], what)
        dy2, dg2 = ops.layerscale_bwd(k["dt"], k["y"], k["gamma"])
        assert torch.equal(dy, dy2) and torch.equal(dg, dg2), what + ": second call differs"
        dgo = InPlace(k["dg0"])
        dy3, dg3 = ops.layerscale_bwd(k["dt"], k["y"], k["gamma"], dg_out=dgo.t, accumulate=True)
        assert dg3 is dgo.t
        S.check_layerscale_bwd(dy3, dgo.ok(what + " dg_out"), k["dt"], k["y"], k["gamma"], what + " accumulate", dg0=k["dg0"])


PAST_CAP = (8200, 1024)            # 8,396,800 elements > 4096 x 256 x 8 = 8,388,608 per sweep


assert PAST_CAP[0] * PAST_CAP[1] > SWEEP


@pytest.mark.parametrize("rows,c", [(7, 384), (2100, 384), (7, 768), (2100, 768), (7, 1024), (2100, 1024), PAST_CAP])
def test_layerscale_bwd_dx_equals_layerscale_bwd(rows, c, guarded):
    ops = _ops()
    k = S.to_dev(S.ls_case(rows, c), DEV)
    what = "rows %d width %d" % (rows, c)
    dy = ops.layerscale_bwd_dx(k["dt"], k["gamma"])
    assert dy.dtype == BF and dy.shape == k["dt"].shape
    assert torch.equal(dy[-1], S.layerscale_dy(k["dt"][-1], k["gamma"])), what + ": last row"
    assert torch.equal(dy, S.layerscale_dy(k["dt"], k["gamma"])), what + ": dy is not bf16(gamma * dt)"
    full, dg = ops.layerscale_bwd(k["dt"], k["y"], k["gamma"])
    assert torch.equal(dy, full), what + ": differs from layerscale_bwd's dy"
    assert torch.equal(dy, ops.layerscale_bwd_dx(k["dt"], k["gamma"])), what + ": second call differs"
    S.check_layerscale_bwd(full, dg, k["dt"], k["y"], k["gamma"], what)


@pytest.mark.parametrize("rows,c", [(5, 384), (5, 1536), PAST_CAP])
def test_scale_residual(rows, c, figs):
    ops = _ops()
    k = S.to_dev(S.ls_case(rows, c), DEV)                       # dt as the stream, y the branch output, gamma the LayerScale
    what = "rows %d width %d" % (rows, c)
    x, x2 = InPlace(k["dt"]), InPlace(k["dt"])
    assert ops.scale_residual_(x.t, k["y"], k["gamma"]) is x.t
    ops.scale_residual_(x2.t, k["y"], k["gamma"])
    S.check_scale_residual(x.ok(what), k["dt"], k["y"], k["gamma"], what)
    assert torch.equal(x.t, x2.ok(what)), what + ": second call differs"


# ---- GELU ----------------------------------------------------------------------------------------------------------------------------------
def test_gelu_every_finite_bf16(guarded):
    ops = _ops()
    x = S.all_finite_bf16().to(DEV)
    assert x.numel() == 65280
    y = ops.gelu(x)
    S.check_gelu(y, x, "gelu")
    assert torch.equal(y, ops.gelu(x)), "second call differs"


@pytest.mark.parametrize("name", ["1", "-0.75", "random"])
def test_gelu_bwd_every_finite_bf16(name, guarded):
    ops = _ops()
    x = S.all_finite_bf16().to(DEV)
    dy = S.gelu_dys(x.numel())[name].to(DEV)
    dx = ops.gelu_bwd(dy, x)
    S.check_gelu_bwd(dx, dy, x, "gelu_bwd dy=" + name)
    assert torch.equal(dx, ops.gelu_bwd(dy, x)), "second call differs"


def test_gelu_past_the_cap(guarded):
    ops = _ops()
    n = SWEEP + 8 * 777
    x = (torch.randn(n, generator=torch.Generator().manual_seed(17)) * 2).to(BF).to(DEV)
    y = ops.gelu(x)
    S.check_gelu(y[-8:], x[-8:], "gelu past the cap, last eight")
    S.check_gelu(y, x, "gelu past the cap")


# ---- softmax -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", S.SOFTMAX_COLS)
def test_softmax_rows(cols, guarded):
    ops = _ops()
    for rows in S.SOFTMAX_ROWS:
        for kind in S.SOFTMAX_KINDS:
            s = S.softmax_case(kind, rows, cols).to(DEV)
            what = "%s rows %d cols %d" % (kind, rows, cols)
            p = ops.softmax_rows_bf16(s, S.SOFTMAX_SCALE)
            S.check_softmax(p, s, S.SOFTMAX_SCALE, what)
            assert torch.equal(p, ops.softmax_rows_bf16(s, S.SOFTMAX_SCALE)), what + ": second call differs"
            if kind == "equal":
                assert torch.equal(p, torch.tensor(1.0 / cols, dtype=F32).to(BF).to(DEV).expand(rows, cols)), what + ": not uniform"
            if kind in ("dominant", "floor"):
                assert torch.equal(p.float().sum(-1), torch.ones(rows, device=DEV)) and bool((p.float().amax(-1) == 1).all()), what + ": not one-hot"


# ---- argument checks: an error code before any launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [128, 640, 1792])
def test_layernorm_entries_refuse_other_widths(c):
    from dmvae_amd._lib import DmvaeHipError
    ops = _ops()
    g = torch.Generator().manual_seed(c)
    x, dres = torch.randn(5, c, generator=g).to(DEV), torch.randn(5, c, generator=g).to(DEV)
    r = torch.randn(5, c, generator=g).to(BF).to(DEV)
    gamma, beta = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    xi, dx = InPlace(x), InPlace(dres)
    with pytest.raises(DmvaeHipError):
        ops.layernorm_bf16(x, gamma, beta)
    with pytest.raises(DmvaeHipError):
        ops.scale_residual_layernorm_(xi.t, r, gamma, gamma, beta)
    with pytest.raises(DmvaeHipError):
        ops.layernorm_bwd_(dx.t, r, x, gamma)
    torch.cuda.synchronize()
    assert torch.equal(xi.ok("refused"), x) and torch.equal(dx.ok("refused"), dres), "a refused call wrote"


def test_softmax_refuses_513_columns():
    from dmvae_amd._lib import DmvaeHipError
    with pytest.raises(DmvaeHipError):
        _ops().softmax_rows_bf16(torch.zeros(3, 513, dtype=BF, device=DEV), S.SOFTMAX_SCALE)
