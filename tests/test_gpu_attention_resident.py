"""The resident attention kernels (csrc/attention.hip, csrc/attention_bwd.hip; S <= 288) through their C entries, in every launch form, against the fp64
definitions and per-element bars of tests/attention_spec.py (-m gpu).  The references run on the GPU in torch double.  Every output is allocated here with a guard
region behind it and pre-filled with 0xFF bytes (NaN in bf16 and f32): the guard must come back untouched, no NaN may survive in the live region, and padded
channels of head-major dq / dk must be exact zeros.  Every call is repeated and must give the same bits.  The backward calls take the forward kernel's own out
and lse, as training does; the bars account for both (attention_spec: E_delta, eps_b).

Which kernel a case launches (launch() in attention_bwd.hip, launch_attention() in attention.hip; BH = batch * heads):
  forward    attention_kernel<64 | 96>; <96, false, true> (persistent) for staged width 96 at BH >= 2 * (CU count rounded down to 8)
  backward   no lse: attention_bwd_kernel<64 | 96>.  With lse: attention_bwd_lse_tight_kernel for d = 72, S <= 256, BH >= 512; else attention_bwd_lse3_kernel<.>
             for S <= 256, BH <= 512; else attention_bwd_lse_kernel<.> (S > 256, or BH > 512)
  test_heads_layout / test_packed_layout (BH = 6 / 4): the one-item forward, attention_bwd_kernel, lse3 up to 256 tokens and attention_bwd_lse_kernel<64 | 96> above
  test_many_blocks: attention_bwd_lse_kernel<64> and <96> at 520 blocks, the tight kernel at 512 and 520 blocks, the persistent forward walking two and three items

Worst |err| / bound observed on an MI355X (bar 1; over every element of every case), per entry and launch form:
  heads   attention_kernel<64> out 0.744, lse 0.050; <96> out 0.732, lse 0.044
          attention_bwd_kernel<64> dq 0.334, dk 0.388, dv 0.876; <96> dq 0.216, dk 0.277, dv 0.819
          attention_bwd_lse3_kernel<64> dq 0.334, dk 0.342, dv 0.831; <96> dq 0.216, dk 0.245, dv 0.784
          attention_bwd_lse_kernel<64> (S >= 257) dq 0.267, dk 0.388, dv 0.876; <96> dq 0.214, dk 0.277, dv 0.819
  packed  attention_kernel<64> out 0.713, lse 0.046; attention_bwd_kernel<64> dq 0.232, dk 0.312, dv 0.838; attention_bwd_lse3_kernel<64> dq 0.207, dk 0.249,
          dv 0.817; attention_bwd_lse_kernel<64> dq 0.232, dk 0.312, dv 0.838
  many    attention_kernel<64> (520 blocks) out 0.794, lse 0.025; attention_kernel<96, persistent> out 0.804, lse 0.024
  blocks  attention_bwd_lse_kernel<64> dq 0.220, dk 0.255, dv 0.809; <96> dq 0.218, dk 0.275, dv 0.797; attention_bwd_lse_tight_kernel dq 0.270, dk 0.268, dv 0.833
  NR      attention_kernel<64, NR> out 0.482; <96, NR> out 0.574 (the figures of the CPU emulation, digit for digit)
The figures are those of the f32 / bf16 emulations of tests/test_attention_spec_cpu.py (out 0.744, lse 0.065, dq 0.334, dk 0.388, dv 0.876).
Every large call equals its samples' small calls bit for bit; no test found a kernel at fault.
"""
import math

import pytest
import torch

import attention_spec as A
from attention_spec import BF, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096          # bytes behind every output
EPS = 1e-6


def _api():
    from dmvae_amd import _lib, ops
    return _lib.lib(), ops


@pytest.fixture
def figs():
    A.FIG.clear()
    yield A.FIG
    for k, v in A.FIG.items():
        print("[fig] %s: worst |err| / bound %.3f (bar 1)" % (k, v))


class Out:
    """an output of `shape`: 0xFF-filled bytes, GUARD more behind them"""

    def __init__(self, shape, dtype):
        self.n = int(math.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.t = self.raw[:self.n].view(dtype).view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def ok(self, what):
        assert bool((self.raw[self.n:] == 0xFF).all()), what + ": written past the output"
        assert not bool(torch.isnan(self.t).any()), what + ": pre-fill survives in the live region (or a NaN was written)"
        return self.t

    def untouched(self, what):
        assert bool((self.raw == 0xFF).all()), what + ": a refused call wrote"


def fwd_form(d, qd, bh):
    dp = A.staged(qd)
    cus = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    return "attention_kernel<96, persistent>" if dp == 96 and bh >= 2 * cus else "attention_kernel<%d>" % dp


def bwd_form(s, d, qd, bh, lse):
    dp = A.staged(qd)
    if not lse:
        return "attention_bwd_kernel<%d>" % dp
    if dp == 96 and d == 72 and s <= 256 and bh >= 512:
        return "attention_bwd_lse_tight_kernel"
    return ("attention_bwd_lse3_kernel<%d>" if s <= 256 and bh <= 512 else "attention_bwd_lse_kernel<%d>") % dp


# ---- the entries, outputs allocated here -----------------------------------------------------------------------------------------------------
def heads_fwd(q, k, v, b, h, d, scale, what, want_lse=True):
    """q, k [G, S, qd], v [G, S, d] -> (out [G, S, d] view of the [B, S, H d] result, lse [G, S] or None)"""
    L, ops = _api()
    s, qd = q.shape[1], q.shape[2]
    out, lse = Out((b, s, h * d), BF), Out((b * h, s), F32) if want_lse else None
    ops.check(L.dmvae_attention_heads_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.ptr(), lse.ptr() if lse else None, b, s, h, d, qd, float(scale),
                                               ops._stream()), "attention_heads_bf16")
    return out.ok(what + " out"), lse.ok(what + " lse") if lse else None


def heads_bwd(q, k, v, o_rows, do_rows, lse, b, h, d, scale, what):
    """-> dq, dk [G, S, qd], dv [G, S, d]"""
    L, ops = _api()
    s, qd = q.shape[1], q.shape[2]
    dq, dk, dv = Out(q.shape, BF), Out(k.shape, BF), Out(v.shape, BF)
    ops.check(L.dmvae_attention_bwd_heads_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o_rows.data_ptr(), do_rows.data_ptr(), lse.data_ptr() if lse is not None else None,
                                                   dq.ptr(), dk.ptr(), dv.ptr(), b, s, h, d, qd, float(scale), ops._stream()), "attention_bwd_heads_bf16")
    dq, dk, dv = dq.ok(what + " dq"), dk.ok(what + " dk"), dv.ok(what + " dv")
    if qd > d:
        assert float(dq[..., d:].float().abs().max()) == 0 and float(dk[..., d:].float().abs().max()) == 0, what + ": padded channels of dq / dk are not exact zeros"
    return dq, dk, dv


def packed_fwd(qkv, b, h, scale, what):
    L, ops = _api()
    s, d = qkv.shape[1], qkv.shape[2] // (3 * h)
    out, lse = Out((b, s, h * d), BF), Out((b * h, s), F32)
    ops.check(L.dmvae_attention_qkv_lse_bf16(qkv.data_ptr(), out.ptr(), lse.ptr(), b, s, h, d, float(scale), ops._stream()), "attention_qkv_bf16")
    out2 = Out((b, s, h * d), BF)
    ops.check(L.dmvae_attention_qkv_lse_bf16(qkv.data_ptr(), out2.ptr(), None, b, s, h, d, float(scale), ops._stream()), "attention_qkv_bf16")
    assert torch.equal(out.t, out2.ok(what + " out (no lse)")), what + ": the form without lse gives other bits"
    return out.ok(what + " out"), lse.ok(what + " lse")


def packed_bwd(qkv, o_rows, do_rows, lse, b, h, scale, what):
    L, ops = _api()
    s, d = qkv.shape[1], qkv.shape[2] // (3 * h)
    dqkv = Out(qkv.shape, BF)
    ops.check(L.dmvae_attention_bwd_qkv_lse_bf16(qkv.data_ptr(), o_rows.data_ptr(), do_rows.data_ptr(), lse.data_ptr() if lse is not None else None, dqkv.ptr(), b, s, h, d,
                                                 float(scale), ops._stream()), "attention_bwd_qkv_bf16")
    return dqkv.ok(what + " dqkv")


def _bars(c):
    ref = A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"])
    fwd = A.bars_forward(c["q"], c["k"], c["v"], c["scale"], ref)
    return ref, fwd, A.bars_backward(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd)


def _hold_grads(got, ref, bwd, what, form):
    for n, g in zip(("dq", "dk", "dv"), got):
        A.hold(g, ref[n], bwd[n], "%s %s" % (what, n), "%s %s" % (form, n))


# ---- both layouts at every token count ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", A.TOKENS)
@pytest.mark.parametrize("d,qd", A.HEAD_FORMS)
def test_heads_layout(d, qd, s, figs):
    b, h = 2, 3
    for kind in A.classes_at(s):
        c = A.to_dev(A.make_case(kind, b, h, s, d), DEV)
        what = "heads %s S %d d %d rows %d" % (kind, s, d, qd)
        ref, fwd, bwd = _bars(c)
        A.check_class(c, ref)
        q, k, do_rows = A.pad_rows(c["q"], qd), A.pad_rows(c["k"], qd), A.to_rows(c["do"], b, h)
        out, lse = heads_fwd(q, k, c["v"], b, h, d, c["scale"], what)
        ff = "heads " + fwd_form(d, qd, b * h)
        A.hold(A.from_rows(out, b, h), ref["o"], fwd["o"], what + " out", ff + " out")
        A.hold(lse, ref["lse"], fwd["lse"], what + " lse", ff + " lse")
        out2, lse2 = heads_fwd(q, k, c["v"], b, h, d, c["scale"], what + " rerun")
        out3, _ = heads_fwd(q, k, c["v"], b, h, d, c["scale"], what + " no lse", want_lse=False)
        assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(out, out3), what + ": forward rerun / the form without lse differ"
        for l in (None, lse):
            g = heads_bwd(q, k, c["v"], out, do_rows, l, b, h, d, c["scale"], what)
            _hold_grads([t[..., :d] for t in g], ref, bwd, what, "heads " + bwd_form(s, d, qd, b * h, l is not None))
            g2 = heads_bwd(q, k, c["v"], out, do_rows, l, b, h, d, c["scale"], what + " rerun")
            assert all(torch.equal(x, y) for x, y in zip(g, g2)), what + ": backward rerun differs"


@pytest.mark.parametrize("s", A.TOKENS)
def test_packed_layout(s, figs):
    b, h, d = 2, 2, 64
    for kind in A.classes_at(s):
        c = A.to_dev(A.make_case(kind, b, h, s, d, seed=1), DEV)
        what = "packed %s S %d" % (kind, s)
        ref, fwd, bwd = _bars(c)
        A.check_class(c, ref)
        qkv, do_rows = A.to_packed(c["q"], c["k"], c["v"], b, h), A.to_rows(c["do"], b, h)
        out, lse = packed_fwd(qkv, b, h, c["scale"], what)
        A.hold(A.from_rows(out, b, h), ref["o"], fwd["o"], what + " out", "packed attention_kernel<64> out")
        A.hold(lse, ref["lse"], fwd["lse"], what + " lse", "packed attention_kernel<64> lse")
        out2, lse2 = packed_fwd(qkv, b, h, c["scale"], what + " rerun")
        assert torch.equal(out, out2) and torch.equal(lse, lse2), what + ": forward rerun differs"
        for l in (None, lse):
            dqkv = packed_bwd(qkv, out, do_rows, l, b, h, c["scale"], what)
            _hold_grads(A.from_packed(dqkv, b, h), ref, bwd, what, "packed " + bwd_form(s, d, d, b * h, l is not None))
            assert torch.equal(dqkv, packed_bwd(qkv, out, do_rows, l, b, h, c["scale"], what + " rerun")), what + ": backward rerun differs"


# ---- the launch forms that the block count selects ---------------------------------------------------------------------------------------------
def _pipe_blocks():
    return 2 * (torch.cuda.get_device_properties(0).multi_processor_count & ~7) + 40


MANY = [(64, 64, 520, 33), (96, 96, 520, 33)]                                                                  # attention_bwd_lse_kernel<64>, <96> above 512 blocks
MANY += [(72, qd, bh, s) for bh in (512, 520) for s in (33, 129, 200, 256) for qd in (72, 96)]                  # the tight kernel; a wave's second block from S > 128
MANY += [(72, qd, "pipe", s) for s in (33, 272) for qd in (72, 96)]                                            # the persistent forward; attention_bwd_lse_kernel<96> at 272


@pytest.mark.parametrize("d,qd,bh,s", MANY)
def test_many_blocks(d, qd, bh, s, figs):
    """Every item (S = 33) or spread_items (larger S) against fp64, and EVERY sample of the large call bit for bit against the same samples run in calls of at most
    496 blocks: out, lse, dq, dk, dv."""
    h = 8
    pipe = bh == "pipe"
    bh = _pipe_blocks() if pipe else bh
    assert not pipe or fwd_form(d, qd, bh).endswith("persistent>")
    b = bh // h
    assert b * h == bh
    for kind in (("randn", "negative") if s == 33 else ("randn",)):
        c = A.make_case(kind, b, h, s, d, seed=2)
        what = "%s %d blocks S %d d %d rows %d" % (kind, bh, s, d, qd)
        q, k, v, do_rows = A.pad_rows(c["q"], qd).to(DEV), A.pad_rows(c["k"], qd).to(DEV), c["v"].to(DEV), A.to_rows(c["do"], b, h).to(DEV)
        out, lse = heads_fwd(q, k, v, b, h, d, c["scale"], what)
        g = heads_bwd(q, k, v, out, do_rows, lse, b, h, d, c["scale"], what)
        ff, bf_ = fwd_form(d, qd, bh), bwd_form(s, d, qd, bh, True)
        if bh >= 512 and d == 72 and s <= 256:
            assert bf_ == "attention_bwd_lse_tight_kernel"
        items = torch.tensor(list(range(bh)) if s == 33 else A.spread_items(bh), device=DEV)
        sub = {n: c[n].to(DEV)[items] for n in ("q", "k", "v", "do")}
        sub["scale"] = c["scale"]
        ref, fwd, bwd = _bars(sub)
        A.hold(A.from_rows(out, b, h)[items], ref["o"], fwd["o"], what + " out", "many blocks %s out" % ff)
        A.hold(lse[items], ref["lse"], fwd["lse"], what + " lse", "many blocks %s lse" % ff)
        _hold_grads([t[items][..., :d] for t in g], ref, bwd, what, "many blocks " + bf_)
        step = 496 // h
        for b0 in range(0, b, step):
            b1 = min(b, b0 + step)
            sl = slice(b0 * h, b1 * h)
            o_c, l_c = heads_fwd(q[sl], k[sl], v[sl], b1 - b0, h, d, c["scale"], what + " chunk")
            assert torch.equal(out[b0:b1], o_c) and torch.equal(lse[sl], l_c), what + ": forward of samples %d..%d differs from the small call" % (b0, b1 - 1)
            g_c = heads_bwd(q[sl], k[sl], v[sl], o_c, do_rows[b0:b1], l_c, b1 - b0, h, d, c["scale"], what + " chunk")
            assert all(torch.equal(x[sl], y) for x, y in zip(g, g_c)), what + ": backward of samples %d..%d differs from the small call" % (b0, b1 - 1)


# ---- the NR entry ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 33, 256, 288])
@pytest.mark.parametrize("d", [64, 72])
def test_qknorm_rope_entry(d, s, figs):
    L, ops = _api()
    b, h = 2, 3
    c = A.make_case("randn", b, h, s, d, seed=5)
    what = "NR S %d d %d" % (s, d)
    qkv = A.to_packed(c["q"], c["k"], c["v"], b, h).to(DEV)
    qw, kw, cos, sin = (t.to(DEV) for t in A.nr_tables(s, d, 0))
    q, k, v, dq_, dk_ = A.nr_operands(qkv, qw, kw, cos, sin, h, EPS)
    ref = A.reference(q, k, v, c["do"].to(DEV), c["scale"])
    fwd = A.bars_forward(q, k, v, c["scale"], ref, dqk=(dq_, dk_))
    outs = []
    for _ in range(2):
        out = Out((b, s, h * d), BF)
        ops.check(L.dmvae_attention_qknorm_rope_bf16(qkv.data_ptr(), qw.data_ptr(), kw.data_ptr(), cos.data_ptr(), sin.data_ptr(), out.ptr(), b, s, h, d, EPS,
                                                     float(c["scale"]), ops._stream()), "attention_qknorm_rope_bf16")
        outs.append(out.ok(what))
    assert torch.equal(outs[0], outs[1]), what + ": rerun differs"
    A.hold(A.from_rows(outs[0], b, h), ref["o"], fwd["o"], what, "NR attention_kernel<%d, NR> out" % A.staged(d))


# ---- refusals: an error code before any launch, nothing written --------------------------------------------------------------------------------
BAD_SCALES = [0.0, -0.125, float("inf"), float("-inf"), float("nan")]
BAD_SHAPES = [(289, 64, 64), (33, 36, 36), (33, 104, 104), (33, 72, 80)]      # (S, d, channels a q / k row holds)


def _refusal_operands(s, d, qd, b=2, h=2):
    g = torch.Generator().manual_seed(s + d)
    mk = lambda *sh: torch.randn(*sh, generator=g).to(BF).to(DEV)
    return mk(b * h, s, qd), mk(b * h, s, qd), mk(b * h, s, d), mk(b, s, h * d), mk(b, s, h * d), torch.zeros(b * h, s, device=DEV)


def _heads_calls_refuse(s, d, qd, scale):
    from dmvae_amd._lib import DmvaeHipError
    L, ops = _api()
    b, h = 2, 2
    q, k, v, o, do, lse = _refusal_operands(s, d, qd)
    out, lo = Out(o.shape, BF), Out(lse.shape, F32)
    with pytest.raises(DmvaeHipError):
        ops.check(L.dmvae_attention_heads_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.ptr(), lo.ptr(), b, s, h, d, qd, scale, ops._stream()), "attention_heads_bf16")
    dq, dk, dv = Out(q.shape, BF), Out(k.shape, BF), Out(v.shape, BF)
    for l in (None, lse.data_ptr()):
        with pytest.raises(DmvaeHipError):
            ops.check(L.dmvae_attention_bwd_heads_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), l, dq.ptr(), dk.ptr(), dv.ptr(), b, s, h, d, qd,
                                                           scale, ops._stream()), "attention_bwd_heads_bf16")
    torch.cuda.synchronize()
    for t in (out, lo, dq, dk, dv):
        t.untouched("heads S %d d %d rows %d scale %r" % (s, d, qd, scale))


@pytest.mark.parametrize("s,d,qd", BAD_SHAPES)
def test_heads_entries_refuse_shapes(s, d, qd):
    _heads_calls_refuse(s, d, qd, d ** -0.5)


@pytest.mark.parametrize("scale", BAD_SCALES)
def test_heads_entries_refuse_scale(scale):
    _heads_calls_refuse(33, 72, 72, scale)


@pytest.mark.parametrize("s,d,scale", [(289, 64, 0.125), (33, 72, 72 ** -0.5)] + [(33, 64, x) for x in BAD_SCALES])
def test_packed_entries_refuse(s, d, scale):
    from dmvae_amd._lib import DmvaeHipError
    L, ops = _api()
    b, h = 2, 2
    g = torch.Generator().manual_seed(s)
    qkv = torch.randn(b, s, 3 * h * d, generator=g).to(BF).to(DEV)
    o, do, lse = qkv[..., :h * d].contiguous(), qkv[..., h * d:2 * h * d].contiguous(), torch.zeros(b * h, s, device=DEV)
    out, lo, dqkv = Out(o.shape, BF), Out(lse.shape, F32), Out(qkv.shape, BF)
    with pytest.raises(DmvaeHipError):
        ops.check(L.dmvae_attention_qkv_lse_bf16(qkv.data_ptr(), out.ptr(), lo.ptr(), b, s, h, d, scale, ops._stream()), "attention_qkv_bf16")
    for l in (None, lse.data_ptr()):
        with pytest.raises(DmvaeHipError):
            ops.check(L.dmvae_attention_bwd_qkv_lse_bf16(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), l, dqkv.ptr(), b, s, h, d, scale, ops._stream()), "attention_bwd_qkv_bf16")
    torch.cuda.synchronize()
    for t in (out, lo, dqkv):
        t.untouched("packed S %d d %d scale %r" % (s, d, scale))


@pytest.mark.parametrize("s,d,scale", [(289, 64, 0.125), (33, 36, 36 ** -0.5), (33, 104, 104 ** -0.5)] + [(33, 72, x) for x in BAD_SCALES])
def test_qknorm_rope_entry_refuses(s, d, scale):
    from dmvae_amd._lib import DmvaeHipError
    L, ops = _api()
    b, h = 2, 2
    qkv = torch.randn(b, s, 3 * h * d, generator=torch.Generator().manual_seed(s + d)).to(BF).to(DEV)
    qw, kw, cos, sin = (t.to(DEV) for t in A.nr_tables(s, d, 0))
    out = Out((b, s, h * d), BF)
    with pytest.raises(DmvaeHipError):
        ops.check(L.dmvae_attention_qknorm_rope_bf16(qkv.data_ptr(), qw.data_ptr(), kw.data_ptr(), cos.data_ptr(), sin.data_ptr(), out.ptr(), b, s, h, d, EPS, scale,
                                                     ops._stream()), "attention_qknorm_rope_bf16")
    torch.cuda.synchronize()
    out.untouched("NR S %d d %d scale %r" % (s, d, scale))
