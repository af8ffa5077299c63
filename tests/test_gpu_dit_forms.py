"""Every launch form of the LightningDiT elementwise kernels (csrc/dit.hip) against the fp64 definitions and element-wise bars of tests/dit_kernels_spec.py (-m gpu).
Each output lies inside a sentinel-filled buffer with guards before and after it (dmod: the columns outside the written chunks), the reference runs on the GPU in
torch double, and every case asserts that a second call gives the same bits.  Which case launches which instantiation: the table in each test's docstring."""
import math

import pytest
import torch

import dit_kernels_spec as S
from dit_kernels_spec import BF, EPS

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -768.0          # exact in bf16 and f32; no case produces it


class Guarded:
    """A tensor of `shape` inside a flat sentinel-filled buffer: guard | payload | guard (each guard at least two rows and 256 elements, a multiple of 64)."""

    def __init__(self, shape, dtype, init=None):
        n = math.prod(shape)
        self.g = (max(256, 2 * shape[-1]) + 63) // 64 * 64
        self.buf = torch.full((2 * self.g + n,), SENT, dtype=dtype, device=DEV)
        self.t = self.buf[self.g:self.g + n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def ok(self, what):
        assert bool((self.buf[:self.g] == SENT).all()), what + ": written before the output"
        assert bool((self.buf[self.g + self.t.numel():] == SENT).all()), what + ": written past the output"
        return self.t


def to_dev(c):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}


def lib():
    from dmvae_amd import _lib
    return _lib.lib()


def call(name, *args):
    from dmvae_amd import _lib, ops
    _lib.check(getattr(lib(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], ops._stream()), name)


def refused(fn, *outputs):
    """fn must raise DmvaeHipError and leave every Guarded output at the sentinel (nothing launched)."""
    from dmvae_amd._lib import DmvaeHipError
    with pytest.raises(DmvaeHipError):
        fn()
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o.buf == SENT).all())


# ---- RMSNorm forward -------------------------------------------------------------------------------------------------------------------
def _rms_fwd(c, shift, y):
    b, n, w_ = c["x"].shape
    call("dmvae_rmsnorm_modulate_bf16", c["x"], c["w"], c["mod"], y, b * n, n, w_, c["mod"].shape[1], c["shift_off"] if shift else -1, c["scale_off"], EPS)


def _rms_gated(c, shift, x, y):
    b, n, w_ = c["x"].shape
    call("dmvae_gated_residual_rmsnorm_modulate", x, c["r"], c["gmod"], c["gmod"].shape[1], c["gate_off"], c["w"], c["mod"], y, b * n, n, w_, c["mod"].shape[1],
         c["shift_off"] if shift else -1, c["scale_off"], EPS)


def _rms_out(c, shift, xo, y):
    b, n, w_ = c["x"].shape
    if y is None:
        call("dmvae_gated_residual_out", c["x"], xo, c["r"], c["gmod"], c["gmod"].shape[1], c["gate_off"], None, None, None, b * n, n, w_, 0, -1, 0, EPS)
    else:
        call("dmvae_gated_residual_out", c["x"], xo, c["r"], c["gmod"], c["gmod"].shape[1], c["gate_off"], c["w"], c["mod"], y, b * n, n, w_, c["mod"].shape[1],
             c["shift_off"] if shift else -1, c["scale_off"], EPS)


@pytest.mark.parametrize("case", S.RMS_FWD, ids=S.case_id)
def test_rmsnorm_forward_forms(case):
    """All three entries through csrc/dit.hip::rmsnorm_modulate_launch<RES>: dmvae_rmsnorm_modulate_bf16 -> rmsnorm_modulate{8}_kernel<false, SW>,
    dmvae_gated_residual_rmsnorm_modulate and dmvae_gated_residual_out -> <true, SW>.
    Four channels per lane (c % 8 != 0, or an offset / stride that is 4 mod 8): SW = ceil(c / 256) -> 1: c 4, 252; 2: 260, 508; 3: 516, 764; 4: 772, 1020; 5: 1028,
    1276 and 1152 with the misaligned chunks; 6: 1284, 1532; 7: 1540, 1788; 8: 1796, 2044.  Eight per lane: SW8 = ceil(c / 512) -> 1: 8, 512; 2: 520, 768,
    1024; 3: 1032, 1152, 1536; 4: 1544, 2048.  15 rows: the last block has 3 live waves and the sample changes inside a block."""
    c = to_dev(S.rms_case(**case))
    shape, w_ = c["x"].shape, c["c"]
    gate = S.chunk(c["gmod"], c["gate_off"], w_)
    scale = S.chunk(c["mod"], c["scale_off"], w_)
    x_new = S.gated_residual_exact(c["x"], gate, c["r"])
    for shift in (True, False):
        sh = S.chunk(c["mod"], c["shift_off"], w_) if shift else None
        what = "%s shift=%s" % (S.case_id(case), shift)
        y, y2 = Guarded(shape, BF), Guarded(shape, BF)
        _rms_fwd(c, shift, y.t); _rms_fwd(c, shift, y2.t)
        S.check_rmsnorm_modulate(y.ok(what), c["x"], c["w"], scale, sh, what=what)
        assert torch.equal(y.t, y2.ok(what)), what + ": second call differs"
        if case.get("hard") and shift:
            assert torch.equal(y.t[0, 0], sh[0]), what + ": the all-zero row must give the shift"
        # in place
        x, x2, y, y2 = Guarded(shape, torch.float32, c["x"]), Guarded(shape, torch.float32, c["x"]), Guarded(shape, BF), Guarded(shape, BF)
        _rms_gated(c, shift, x.t, y.t); _rms_gated(c, shift, x2.t, y2.t)
        assert torch.equal(x.ok(what), x_new), what + ": residual stream (in place)"
        S.check_rmsnorm_modulate(y.ok(what), x_new, c["w"], scale, sh, what=what + " fused")
        assert torch.equal(x.t, x2.ok(what)) and torch.equal(y.t, y2.ok(what)), what + ": second call differs (in place)"
        # out of place, with and without the norm
        xin = c["x"].clone()
        xo, y3, xo2 = Guarded(shape, torch.float32), Guarded(shape, BF), Guarded(shape, torch.float32)
        _rms_out(c, shift, xo.t, y3.t); _rms_out(c, shift, xo2.t, None)
        assert torch.equal(c["x"], xin), what + ": the input of the out-of-place form changed"
        assert torch.equal(xo.ok(what), x_new) and torch.equal(xo2.ok(what), x_new), what + ": residual stream (out of place)"
        assert torch.equal(y3.ok(what), y.t), what + ": out-of-place y differs from the in-place form's"
        if case.get("hard"):
            assert torch.equal(xo.t[..., 3::4], c["x"][..., 3::4]), what + ": gate = 0 columns must stay bit-unchanged"
    refused(lambda: call("dmvae_rmsnorm_modulate_bf16", c["x"], c["w"], c["mod"], None, shape[0] * shape[1], shape[1], w_, c["mod"].shape[1], -1, c["scale_off"], EPS))
    x = Guarded(shape, torch.float32, c["x"])
    refused(lambda: call("dmvae_gated_residual_rmsnorm_modulate", x.t, c["r"], c["gmod"], c["gmod"].shape[1], c["gate_off"], c["w"], c["mod"], None,
                         shape[0] * shape[1], shape[1], w_, c["mod"].shape[1], -1, c["scale_off"], EPS))       # y = None: only the out-of-place form takes it
    assert torch.equal(x.ok("refused"), c["x"])


# ---- RMSNorm backward ------------------------------------------------------------------------------------------------------------------
def _rms_bwd(c, shift, accumulate):
    from dmvae_amd import ops
    b, n, w_ = c["x"].shape
    dx = Guarded(c["x"].shape, torch.float32, c["dres"])
    dmod = Guarded(c["mod"].shape, torch.float32)
    dw0 = torch.linspace(-3, 3, w_, device=DEV) if accumulate else None
    dw = Guarded((w_,), torch.float32, dw0)
    ops.rmsnorm_modulate_bwd_(dx.t, c["da"], c["x"], c["w"], c["mod"], dmod.t, c["shift_off"] if shift else -1, c["scale_off"], EPS, dw_out=dw.t, accumulate=accumulate)
    return dx, dmod, dw, dw0


def _rms_bwd_case(case):
    """both routes: with a shift chunk into a fresh dw, and without one accumulating into a dw that holds known values"""
    c = to_dev(S.rms_case(**case))
    w_ = c["c"]
    for shift, accumulate in ((True, False), (False, True)):
        what = "%s shift=%s accumulate=%s" % (S.case_id(case), shift, accumulate)
        dx, dmod, dw, dw0 = _rms_bwd(c, shift, accumulate)
        dx2, dmod2, dw2, _ = _rms_bwd(c, shift, accumulate)
        dm = dmod.ok(what)
        S.check_rmsnorm_modulate_bwd(dx.ok(what), S.chunk(dm, c["shift_off"], w_).contiguous() if shift else None, S.chunk(dm, c["scale_off"], w_).contiguous(),
                                     dw.ok(what), c["dres"], c["da"], c["x"], c["w"], S.chunk(c["mod"], c["scale_off"], w_), dw0=dw0, what=what)
        written = torch.zeros(dm.shape[1], dtype=torch.bool, device=DEV)
        written[c["scale_off"]:c["scale_off"] + w_] = True
        if shift:
            written[c["shift_off"]:c["shift_off"] + w_] = True
        assert bool((dm[:, ~written] == SENT).all()), what + ": dmod written outside its chunks"
        assert torch.equal(dx.t, dx2.ok(what)) and torch.equal(dmod.t, dmod2.ok(what)) and torch.equal(dw.t, dw2.ok(what)), what + ": second call differs"


@pytest.mark.parametrize("case", S.RMS_BWD, ids=S.case_id)
def test_rmsnorm_backward_two_kernel_route(case):
    """dmvae_rmsnorm_modulate_bwd with seq <= 4096: rmsnorm_rowstat_kernel + rmsnorm_modulate_bwd_apply_kernel (64 .. 512 threads: c = 4 -> 64, 2044 / 2048 -> 512) +
    the final and weight kernels.  Blocks per sample: 32 (b = 1, 2, 3: with n = 5 most blocks have no rows), 25 (b = 40), clamped to 4 (b = 300)."""
    _rms_bwd_case(case)


@pytest.mark.parametrize("case", S.RMS_BWD_FALLBACK, ids=S.case_id)
def test_rmsnorm_backward_single_kernel_route(case):
    """dmvae_rmsnorm_modulate_bwd with seq > 4096: rmsnorm_modulate_bwd_kernel<SW>, dynamic LDS 24 c bytes -> SW 1: c 8; 2: 260; 3: 516; 4: 772; 5: 1028; 6: 1284;
    7: 1540; 8: 2048; and two samples at c = 8."""
    _rms_bwd_case(case)


# ---- gated residual --------------------------------------------------------------------------------------------------------------------
def _gated(case):
    from dmvae_amd import ops
    c = to_dev(S.rms_case(hard=True, **case))                       # gate = 0 columns; the gate chunk at 2 c inside a 6 c row
    b, n, w_ = c["x"].shape
    what = S.case_id(case)
    gate = S.chunk(c["gmod"], c["gate_off"], w_)
    x, x2 = Guarded(c["x"].shape, torch.float32, c["x"]), Guarded(c["x"].shape, torch.float32, c["x"])
    ops.gated_residual_(x.t, c["r"], c["gmod"], c["gate_off"]); ops.gated_residual_(x2.t, c["r"], c["gmod"], c["gate_off"])
    assert torch.equal(x.ok(what), S.gated_residual_exact(c["x"], gate, c["r"])), what + ": gated_residual_"
    assert torch.equal(x.t[..., 3::4], c["x"][..., 3::4]) and torch.equal(x.t, x2.ok(what))
    outs = []
    for _ in range(2):
        dy, dmod = Guarded(c["x"].shape, BF), Guarded(c["gmod"].shape, torch.float32)
        call("dmvae_gated_residual_bwd", c["dres"], c["r"], c["gmod"], dy.t, dmod.t, b, n, w_, c["gmod"].shape[1], c["gate_off"])
        outs.append((dy.ok(what), dmod.ok(what)))
    want_dy, dgate, terms = S.gated_residual_bwd(c["dres"], gate, c["r"])
    assert torch.equal(outs[0][0], want_dy), what + ": dy"
    S.check_f32(S.chunk(outs[0][1], c["gate_off"], w_).contiguous(), dgate, terms, S.gated_bwd_depth(n), what + " dgate")
    assert bool((outs[0][1][:, :c["gate_off"]] == SENT).all()) and bool((outs[0][1][:, c["gate_off"] + w_:] == SENT).all()), what + ": dmod written outside the gate chunk"
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("case", S.GATED + [dict(b=2, n=2050, c=2048)], ids=S.case_id)
def test_gated_residual_and_backward(case):
    """gated_residual_kernel (grid capped at 4096 x 256 threads) and gated_residual_bwd_kernel; 4100 x 2048 = 1,049,600 vectors: one whole pass of the grid and a
    ragged second one."""
    _gated(case)


# ---- SwiGLU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.SWIGLU + [dict(rows=2050, hid=4096)], ids=S.case_id)
def test_swiglu_and_backward(case):
    """swiglu_kernel / swiglu_bwd_kernel (grid capped at 4096 x 256 threads); 2050 x 4096 = 1,049,600 vectors, past the cap, a guard after the last row."""
    c = to_dev(S.swiglu_case(hard=True, **case))
    rows, hid, what = case["rows"], case["hid"], S.case_id(case)
    h, h2, g, g2 = Guarded((rows, hid), BF), Guarded((rows, hid), BF), Guarded((rows, 2 * hid), BF), Guarded((rows, 2 * hid), BF)
    for o, d in ((h, g), (h2, g2)):
        call("dmvae_swiglu_bf16", c["x12"], o.t, rows, hid)
        call("dmvae_swiglu_bwd", c["dh"], c["x12"], d.t, rows, hid)
    S.check_swiglu(h.ok(what), c["x12"], what)
    S.check_swiglu_bwd(g.ok(what), c["dh"], c["x12"], what + " bwd")
    assert torch.equal(h.t, h2.ok(what)) and torch.equal(g.t, g2.ok(what)), what + ": second call differs"


# ---- QK-norm + RoPE --------------------------------------------------------------------------------------------------------------------
def _qk(case):
    from dmvae_amd import ops
    c = to_dev(S.qk_case(**case))
    b, n = c["qkv"].shape[:2]
    heads, d, dp, what = c["heads"], c["d"], c["dp"], S.case_id(case)
    fw = []
    for _ in range(2):
        q, k, v = Guarded((b * heads, n, dp), BF), Guarded((b * heads, n, dp), BF), Guarded((b * heads, n, d), BF)
        call("dmvae_qknorm_rope_bf16", c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], q.t, k.t, v.t, b, n, heads, d, dp, EPS)
        fw.append((q.ok(what), k.ok(what), v.ok(what)))
    S.check_qknorm_rope(*fw[0], c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], heads, what=what)
    assert all(torch.equal(a, e) for a, e in zip(*fw)), what + ": second call differs"
    if dp == (d + 31) // 32 * 32:                                # ops pads exactly so
        qo, ko, vo = ops.qknorm_rope(c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], heads)
        assert qo.shape[-1] == dp and torch.equal(qo, fw[0][0]) and torch.equal(ko, fw[0][1]) and torch.equal(vo, fw[0][2])
    if case.get("hard"):
        hq = fw[0][0].view(b, heads, n, dp)[:, heads - 1]
        assert not bool(hq.float().abs().max() > 0), what + ": the zero head's q"
    # backward: the full call, the partial-sum form and the dx-only form
    ws = ops.workspace(lib().dmvae_dit_bwd_workspace(b, heads * d), c["qkv"].device)
    bw = []
    for _ in range(2):
        dqkv, dqw, dkw = Guarded(c["qkv"].shape, BF), Guarded((d,), torch.float32), Guarded((d,), torch.float32)
        call("dmvae_qknorm_rope_bwd", c["dq"], c["dk"], c["dv"], c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], dqkv.t, dqw.t, dkw.t, ws, ws.numel(), b, n, heads, d, dp, EPS, 0)
        bw.append((dqkv.ok(what), dqw.ok(what), dkw.ok(what)))
    o = S.check_qknorm_rope_bwd(*bw[0], c["dq"], c["dk"], c["dv"], c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], heads, what=what)
    assert all(torch.equal(a, e) for a, e in zip(*bw)), what + ": second call differs (backward)"
    st = ops.DitStackBwd(1, b, n, heads * d, heads, c["qkv"].device)
    assert st.nblk == S.qk_bwd_nblk(b * n * heads, d, dp)[0]
    dpart = st.qknorm_rope_bwd(0, c["dq"], c["dk"], c["dv"], c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], EPS)
    assert torch.equal(dpart, bw[0][0]), what + ": the partial-sum form's dqkv differs"
    part = st.qk_part[:st.nblk * 2 * d].view(st.nblk, 2, d).double().sum(0)                          # the blocks' partials, summed in fp64: every block wrote its slot
    depth = S.qk_bwd_dw_depth(b * n * heads, d, dp)
    S.check_f32(part[0].float(), o["dqw"], o["dqw_terms"], depth, what + " partials q", extra=o["dqw_flip"])
    S.check_f32(part[1].float(), o["dkw"], o["dkw_terms"], depth, what + " partials k", extra=o["dkw_flip"])
    sx = ops.DitStackBwd(1, b, n, heads * d, heads, c["qkv"].device, dx_only=True)
    assert torch.equal(sx.qknorm_rope_bwd_dx(c["dq"], c["dk"], c["dv"], c["qkv"], c["qw"], c["kw"], c["cos"], c["sin"], EPS), bw[0][0]), what + ": the dx-only form's dqkv differs"


@pytest.mark.parametrize("case", S.QK_GENERIC + [S.QK_GENERIC_LOOP, S.QK_HARD[0]], ids=S.case_id)
def test_qknorm_rope_generic_kernels(case):
    """head dim % 8 != 0: dmvae_qknorm_rope_bf16 -> qknorm_rope_kernel; qk_bwd_launch -> qknorm_rope_bwd_kernel<true> (full, partial) and <false> (dx only).  Row
    counts 3, 30, 35, 18, 15: no multiple of 4; 8,202 rows: the stride loop past 2048 blocks."""
    _qk(case)


@pytest.mark.parametrize("case", S.QK16 + [S.QK16_LOOP, S.QK_HARD[1]], ids=S.case_id)
def test_qknorm_rope_16_lane_kernels(case):
    """head dim % 8 == 0: qknorm_rope16_kernel; qk_bwd_launch -> qknorm_rope16_bwd_kernel<true> and <false>.  Row counts 9, 30, 21, 5: ragged last block (inr == false,
    row >= rows); Dp = D = 72 and 128 unpadded; 32,800 rows: the stride loop past 2048 blocks."""
    _qk(case)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from dmvae_amd import ops
    g = torch.Generator().manual_seed(0)
    # too wide; not a multiple of 4; shift offset 2; scale chunk past the row; SHIFT chunk past the row (12 + 8 > 16)
    for w_, stride, shift_off, scale_off in ((2052, None, 0, None), (6, None, 0, None), (8, None, 2, None), (8, 12, 0, 8), (8, 16, 12, 0)):
        stride = 6 * w_ if stride is None else stride
        scale_off = w_ if scale_off is None else scale_off
        x, r = torch.randn(2, 3, w_, generator=g).to(DEV), torch.randn(2, 3, w_, generator=g).to(DEV).to(BF)
        w, mod = torch.ones(w_, device=DEV), torch.randn(2, stride, generator=g).to(DEV).to(BF)
        y, xo = Guarded(x.shape, BF), Guarded(x.shape, torch.float32)
        refused(lambda: call("dmvae_rmsnorm_modulate_bf16", x, w, mod, y.t, 6, 3, w_, stride, shift_off, scale_off, EPS), y)
        refused(lambda: call("dmvae_gated_residual_rmsnorm_modulate", xo.t, r, mod, stride, 0, w, mod, y.t, 6, 3, w_, stride, shift_off, scale_off, EPS), y, xo)
        refused(lambda: call("dmvae_gated_residual_out", x, xo.t, r, mod, stride, 0, w, mod, y.t, 6, 3, w_, stride, shift_off, scale_off, EPS), y, xo)
        dx, dmod, dw = Guarded(x.shape, torch.float32), Guarded(mod.shape, torch.float32), Guarded((w_,), torch.float32)
        refused(lambda: ops.rmsnorm_modulate_bwd_(dx.t, r, x, w, mod, dmod.t, shift_off, scale_off, dw_out=dw.t), dx, dmod, dw)
    for d, dp in ((7, 32), (8, 136)):                       # odd head dim; padded head dim above 128
        qkv = torch.randn(1, 3, 3 * 2 * d, generator=g).to(DEV).to(BF)
        ones, tab = torch.ones(d, device=DEV), torch.ones(3, d, device=DEV)
        q, k, v = Guarded((2, 3, dp), BF), Guarded((2, 3, dp), BF), Guarded((2, 3, d), BF)
        refused(lambda: call("dmvae_qknorm_rope_bf16", qkv, ones, ones, tab, tab, q.t, k.t, v.t, 1, 3, 2, d, dp, EPS), q, k, v)
        dqkv = Guarded(qkv.shape, BF)
        refused(lambda: call("dmvae_qknorm_rope_bwd_dx", q.t, k.t, v.t, qkv, ones, ones, tab, tab, dqkv.t, 1, 3, 2, d, dp, EPS), dqkv)
    x = Guarded((2, 3, 12), torch.float32)
    refused(lambda: ops.gated_residual_(x.t, torch.ones(2, 3, 12, device=DEV, dtype=BF), torch.ones(2, 72, device=DEV, dtype=BF), 24), x)
