"""The streaming attention kernels (csrc/attention_stream.hip, csrc/attention_bwd_stream.hip; any S) through their four C entries, in every launch form, against
the fp64 definitions and the per-element streaming bars of tests/attention_spec.py (-m gpu).  The references run on the GPU in torch double.  Every output --
out, lse, dq, dk, dv (dqkv) and delta -- is carved out of a buffer with a guard zone on BOTH sides and pre-filled with 0xFF bytes (NaN in bf16 and f32): the guards
must come back untouched, no NaN may survive in the live region, every element is held to its bar, and padded channels of head-major dq / dk are exact zeros.
The backward runs twice per case: on the forward kernel's own out / lse (the pipeline; bars with the forward's terms) and on bf16(o) / f32(lse) of the
definition, so that a forward defect can neither hide nor cause a backward failure.  Reruns give the same bits; so do the forms with and without lse, q / k rows
of 72 and of 96 channels, a 2B call against two B calls, and -- the same instantiation on other strides, every sum in a fixed order per (sample, head) -- the
packed against the head-major layout at d = 64.

Which kernels a case launches: forward attention_stream_kernel<64 | 96> on B H ceil(S / 256) blocks; backward attention_bwd_stream_dq_kernel<64 | 96> on the same
grid, then attention_bwd_stream_dkdv_kernel<64, 512> on the same grid or <96, 256> on B H ceil(S / 128) blocks.

Worst |err| / bound observed on an MI355X (bar 1; over every element of every case of this module), per entry and output:
  dmvae_attention_qkv_stream_bf16        (packed, <64>)          out 0.746, lse 0.046
  dmvae_attention_heads_stream_bf16      (d 64, <64>)            out 0.746, lse 0.046 -- the packed entry's bits
                                         (d 72, <96>)            out 0.731, lse 0.041, rows of 72 and of 96 alike
  dmvae_attention_bwd_qkv_stream_bf16    (<64> + <64, 512>)      own operands  dq 0.254, dk 0.348, dv 0.850, delta 0.161
                                                                 made operands dq 0.525, dk 0.514, dv 0.891, delta 0.363
  dmvae_attention_bwd_heads_stream_bf16  (d 64)                  the packed entry's bits and figures
                                         (d 72, <96> + <96, 256>) own operands  dq 0.234, dk 0.277, dv 0.801, delta 0.149
                                                                 made operands dq 0.433, dk 0.470, dv 0.854, delta 0.343
The CPU emulations of tests/test_attention_stream_spec_cpu.py reach out 0.726, lse 0.063, dv 0.886 at worst: the kernels sit where their emulations do.  Every
bit-identity above held, every refusal returned an error with nothing written, and no test found a kernel at fault.  The whole module runs in a few seconds.
"""
import math

import pytest
import torch

import attention_spec as A
from attention_spec import BF, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096          # bytes in front of and behind every output


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
    """an output of `shape` between two guard zones, everything filled with 0xFF bytes"""

    def __init__(self, shape, dtype):
        self.n = int(math.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((GUARD + self.n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.n].view(dtype).view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def ok(self, what):
        assert bool((self.raw[:GUARD] == 0xFF).all()), what + ": written in front of the output"
        assert bool((self.raw[GUARD + self.n:] == 0xFF).all()), what + ": written past the output"
        assert not bool(torch.isnan(self.t).any()), what + ": pre-fill survives in the live region (or a NaN was written)"
        return self.t

    def untouched(self, what):
        assert bool((self.raw == 0xFF).all()), what + ": a refused call wrote"


# ---- the four entries, outputs allocated here --------------------------------------------------------------------------------------------------
def packed_fwd(qkv, b, h, scale, what, want_lse=True):
    """qkv [B, S, 3 H 64] -> (out [B, S, H 64], lse [B H, S] or None)"""
    L, ops = _api()
    s, d = qkv.shape[1], qkv.shape[2] // (3 * h)
    out, lse = Out((b, s, h * d), BF), Out((b * h, s), F32) if want_lse else None
    ops.check(L.dmvae_attention_qkv_stream_bf16(qkv.data_ptr(), out.ptr(), lse.ptr() if lse else None, b, s, h, d, float(scale), ops._stream()), "attention_qkv_stream_bf16")
    return out.ok(what + " out"), lse.ok(what + " lse") if lse else None


def heads_fwd(q, k, v, b, h, d, scale, what, want_lse=True):
    """q, k [G, S, qd], v [G, S, d] -> (out [B, S, H d], lse [G, S] or None)"""
    L, ops = _api()
    s, qd = q.shape[1], q.shape[2]
    out, lse = Out((b, s, h * d), BF), Out((b * h, s), F32) if want_lse else None
    ops.check(L.dmvae_attention_heads_stream_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.ptr(), lse.ptr() if lse else None, b, s, h, d, qd, float(scale),
                                                  ops._stream()), "attention_heads_stream_bf16")
    return out.ok(what + " out"), lse.ok(what + " lse") if lse else None


def packed_bwd(qkv, o_rows, do_rows, lse, b, h, scale, what):
    """-> dqkv in qkv's layout, delta [B H, S]"""
    L, ops = _api()
    s, d = qkv.shape[1], qkv.shape[2] // (3 * h)
    dqkv, delta = Out(qkv.shape, BF), Out((b * h, s), F32)
    ops.check(L.dmvae_attention_bwd_qkv_stream_bf16(qkv.data_ptr(), o_rows.data_ptr(), do_rows.data_ptr(), lse.data_ptr(), dqkv.ptr(), delta.ptr(), b, s, h, d, float(scale),
                                                    ops._stream()), "attention_bwd_qkv_stream_bf16")
    return dqkv.ok(what + " dqkv"), delta.ok(what + " delta")


def heads_bwd(q, k, v, o_rows, do_rows, lse, b, h, d, scale, what):
    """-> dq, dk [G, S, qd], dv [G, S, d], delta [G, S]"""
    L, ops = _api()
    s, qd = q.shape[1], q.shape[2]
    dq, dk, dv, delta = Out(q.shape, BF), Out(k.shape, BF), Out(v.shape, BF), Out((b * h, s), F32)
    ops.check(L.dmvae_attention_bwd_heads_stream_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o_rows.data_ptr(), do_rows.data_ptr(), lse.data_ptr(), dq.ptr(), dk.ptr(),
                                                      dv.ptr(), delta.ptr(), b, s, h, d, qd, float(scale), ops._stream()), "attention_bwd_heads_stream_bf16")
    dq, dk, dv, delta = dq.ok(what + " dq"), dk.ok(what + " dk"), dv.ok(what + " dv"), delta.ok(what + " delta")
    assert A.padded_columns_are_zero(dq, d) and A.padded_columns_are_zero(dk, d), what + ": padded channels of dq / dk are not exact zeros"
    return dq, dk, dv, delta


# ---- one form of one case: forward, both backward runs, every bit-identity that needs no second form ---------------------------------------------
class Form:
    """layout "packed" (d = 64) or "heads" with q / k rows of `qd` channels; .fwd / .bwd return everything in the working layout [G, S, .] next to the raw tensors"""

    def __init__(self, layout, c, b, h, qd=None):
        self.layout, self.c, self.b, self.h, self.d = layout, c, b, h, c["d"]
        self.qd = qd or self.d
        self.do_rows = A.to_rows(c["do"], b, h)
        if layout == "packed":
            self.qkv = A.to_packed(c["q"], c["k"], c["v"], b, h)
        else:
            self.q, self.k = A.pad_rows(c["q"], self.qd), A.pad_rows(c["k"], self.qd)
        dp = A.staged(self.d)
        self.name = "%s %s" % (layout, "d 64" if self.d == 64 else "d 72 rows %d" % self.qd)
        self.kernels = ("attention_stream_kernel<%d>" % dp, "attention_bwd_stream_dq_kernel<%d>" % dp, "attention_bwd_stream_dkdv_kernel<%d, %d>" % (dp, 512 if dp == 64 else 256))

    def fwd(self, what, want_lse=True):
        """-> out rows [B, S, H d], lse [G, S]"""
        if self.layout == "packed":
            return packed_fwd(self.qkv, self.b, self.h, self.c["scale"], what, want_lse)
        return heads_fwd(self.q, self.k, self.c["v"], self.b, self.h, self.d, self.c["scale"], what, want_lse)

    def bwd(self, o_rows, lse, what):
        """-> dq, dk, dv [G, S, d], delta [G, S]"""
        if self.layout == "packed":
            dqkv, delta = packed_bwd(self.qkv, o_rows, self.do_rows, lse, self.b, self.h, self.c["scale"], what)
            return tuple(t.contiguous() for t in A.from_packed(dqkv, self.b, self.h)) + (delta,)
        dq, dk, dv, delta = heads_bwd(self.q, self.k, self.c["v"], o_rows, self.do_rows, lse, self.b, self.h, self.d, self.c["scale"], what)
        return dq[..., :self.d].contiguous(), dk[..., :self.d].contiguous(), dv, delta


def _bars(c):
    ref = A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"])
    fwd = A.bars_forward_stream(c["q"], c["k"], c["v"], c["scale"], ref)
    own = A.bars_backward_stream(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd, "kernel")
    made = A.bars_backward_stream(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd, "reference")
    return ref, fwd, own, made


def _hold_grads(got, ref, bars, what, key):
    for n, g in zip(("dq", "dk", "dv"), got[:3]):
        A.hold(g, ref[n], bars[n], "%s %s" % (what, n), "%s %s" % (key, n))
    A.hold(got[3], ref["delta"].squeeze(-1), bars["delta"], what + " delta", key + " delta")


def _same(x, y):
    return all(torch.equal(a, b) for a, b in zip(x, y))


def run_form(f, what, ref, fwd, own, made, items=None, rerun=True):
    """the form's forward and both backward runs held to the bars (every item, or `items`); -> (out rows, lse, grads on own operands, grads on made operands)"""
    b, h = f.b, f.h
    sel = (lambda t: t) if items is None else (lambda t: t[items])
    fk, qk, kk = f.kernels
    out, lse = f.fwd(what)
    A.hold(sel(A.from_rows(out, b, h)), ref["o"], fwd["o"], what + " out", "%s %s out" % (f.name, fk))
    A.hold(sel(lse), ref["lse"], fwd["lse"], what + " lse", "%s %s lse" % (f.name, fk))
    out_n, _ = f.fwd(what + " no lse", want_lse=False)
    assert torch.equal(out, out_n), what + ": the form without lse gives other bits"
    g_own = f.bwd(out, lse, what + " own operands")
    _hold_grads([sel(t) for t in g_own], ref, own, what + " (own operands)", "%s %s + %s (own operands)" % (f.name, qk, kk))
    if items is None:
        o_r, l_r = A.reference_operands(ref)
        g_made = f.bwd(A.to_rows(o_r, b, h), l_r.contiguous(), what + " made operands")
        _hold_grads(g_made, ref, made, what + " (made operands)", "%s %s + %s (made operands)" % (f.name, qk, kk))
    else:
        g_made = None
    if rerun:
        out2, lse2 = f.fwd(what + " rerun")
        assert torch.equal(out, out2) and torch.equal(lse, lse2), what + ": forward rerun differs"
        assert _same(g_own, f.bwd(out, lse, what + " rerun")), what + ": backward rerun differs"
    return out, lse, g_own, g_made


# ---- every token count, both layouts at d = 64 and both row widths at d = 72 --------------------------------------------------------------------------
@pytest.mark.parametrize("s", A.STREAM_TOKENS)
def test_d64_packed_and_heads_layout(s, figs):
    b, h = 2, 3
    for kind in A.stream_classes_at(s):
        c = A.to_dev(A.make_case(kind, b, h, s, 64, seed=1), DEV)
        what = "%s S %d d 64" % (kind, s)
        bars = _bars(c)
        A.check_class(c, bars[0])
        rp = run_form(Form("packed", c, b, h), "packed " + what, *bars)
        rh = run_form(Form("heads", c, b, h), "heads " + what, *bars, rerun=False)
        assert torch.equal(rp[0], rh[0]) and torch.equal(rp[1], rh[1]), what + ": the two layouts' forward bits differ"
        assert _same(rp[2], rh[2]) and _same(rp[3], rh[3]), what + ": the two layouts' backward bits differ"


@pytest.mark.parametrize("s", A.STREAM_TOKENS)
def test_d72_rows_of_72_and_of_96(s, figs):
    b, h = 2, 3
    for kind in A.stream_classes_at(s):
        c = A.to_dev(A.make_case(kind, b, h, s, 72), DEV)
        what = "%s S %d d 72" % (kind, s)
        bars = _bars(c)
        A.check_class(c, bars[0])
        r72 = run_form(Form("heads", c, b, h, 72), "rows 72 " + what, *bars)
        r96 = run_form(Form("heads", c, b, h, 96), "rows 96 " + what, *bars, rerun=False)
        assert torch.equal(r72[0], r96[0]) and torch.equal(r72[1], r96[1]), what + ": the two row widths' forward bits differ"
        assert _same(r72[2], r96[2]) and _same(r72[3], r96[3]), what + ": the two row widths' backward bits differ"


ONCE_1025 = [("packed", 64, None, "randn"), ("heads", 72, 96, "ascending")]      # each of the four entries once


@pytest.mark.parametrize("layout,d,qd,kind", ONCE_1025)
def test_1025_tokens(layout, d, qd, kind, figs):
    b, h = 1, 2
    c = A.to_dev(A.make_case(kind, b, h, 1025, d), DEV)
    bars = _bars(c)
    A.check_class(c, bars[0])
    run_form(Form(layout, c, b, h, qd), "%s %s S 1025 d %d" % (layout, kind, d), *bars)


# ---- block counts: 1, 6, 15, and above 512 behind xcd_remap; heads of 1 and 3 -------------------------------------------------------------------------
# (batch, heads, S, d): forward / query-pass blocks B H ceil(S / 256); the 96-wide key pass has B H ceil(S / 128)
FEW = [(1, 1, 200, 64), (1, 1, 97, 72), (2, 3, 129, 64), (2, 3, 129, 72), (5, 1, 513, 64), (5, 3, 255, 72), (5, 1, 321, 72)]


@pytest.mark.parametrize("b,h,s,d", FEW)
def test_block_counts(b, h, s, d, figs):
    for kind in ("randn", "ascending"):
        c = A.to_dev(A.make_case(kind, b, h, s, d, seed=3), DEV)
        bars = _bars(c)
        for layout in (("packed", "heads") if d == 64 else ("heads",)):
            run_form(Form(layout, c, b, h), "%s %s %d x %d heads S %d d %d" % (layout, kind, b, h, s, d), *bars)


@pytest.mark.parametrize("layout,d,qd", [("packed", 64, None), ("heads", 64, None), ("heads", 72, 96)])
def test_many_blocks(layout, d, qd, figs):
    """260 items at 257 tokens: 520 blocks in the forward and the query pass (780 in the 96-wide key pass).  spread_items against fp64; EVERY sample bit for bit
    against the same samples run 13 at a time -- with the NaN pre-fill and the guards, every (sample, head, block) behind xcd_remap is computed, in its own place."""
    b, h, s = 65, 4, 257
    c = A.make_case("randn", b, h, s, d, seed=2)
    what = "%s %d items S %d d %d" % (layout, b * h, s, d)
    items = torch.tensor(A.spread_items(b * h), device=DEV)
    sub = {n: c[n].to(DEV)[items] for n in ("q", "k", "v", "do")}
    sub.update(scale=c["scale"], d=d)
    cd = A.to_dev(c, DEV)
    f = Form(layout, cd, b, h, qd)
    out, lse, g, _ = run_form(f, what, *_bars(sub), items=items, rerun=False)
    step = 13
    for b0 in range(0, b, step):
        sl = slice(b0 * h, (b0 + step) * h)
        cc = {n: cd[n][sl] for n in ("q", "k", "v", "do")}
        cc.update(scale=c["scale"], d=d)
        fc = Form(layout, cc, step, h, qd)
        o_c, l_c = fc.fwd(what + " chunk")
        assert torch.equal(out[b0:b0 + step], o_c) and torch.equal(lse[sl], l_c), what + ": forward of samples %d.. differs from the small call" % b0
        assert _same([t[sl] for t in g], fc.bwd(o_c, l_c, what + " chunk")), what + ": backward of samples %d.. differs from the small call" % b0


@pytest.mark.parametrize("layout,d,qd,s", [("packed", 64, None, 321), ("heads", 72, 72, 289)])
def test_a_2b_call_equals_two_b_calls(layout, d, qd, s):
    b, h = 4, 3
    c = A.to_dev(A.make_case("randn", b, h, s, d, seed=4), DEV)
    f = Form(layout, c, b, h, qd)
    out, lse = f.fwd("2B")
    g = f.bwd(out, lse, "2B")
    for b0 in (0, 2):
        sl = slice(b0 * h, (b0 + 2) * h)
        cc = {n: c[n][sl] for n in ("q", "k", "v", "do")}
        cc.update(scale=c["scale"], d=d)
        fc = Form(layout, cc, 2, h, qd)
        o_c, l_c = fc.fwd("B")
        assert torch.equal(out[b0:b0 + 2], o_c) and torch.equal(lse[sl], l_c)
        assert _same([t[sl] for t in g], fc.bwd(o_c, l_c, "B"))


# ---- refusals: an error code before any launch, nothing written --------------------------------------------------------------------------------------
BAD_SCALES = [0.0, -0.125, float("inf"), float("-inf"), float("nan")]
# what attn_stream_check refuses besides the scale: (batch, seq, heads, head_dim, channels a q / k row holds); the operands are those of a valid 2 x 33 x 2 call
BAD_HEADS_SHAPES = [(0, 33, 2, 64, 64), (2, 0, 2, 64, 64), (2, 33, 0, 64, 64), (-1, 33, 2, 72, 72), (2, 33, 2, 40, 40), (2, 33, 2, 96, 96), (2, 33, 2, 80, 96),
                    (2, 33, 2, 64, 96), (2, 33, 2, 72, 80), (2, 33, 2, 72, 64), (65536, 33, 65536, 64, 64)]
BAD_PACKED_SHAPES = [(0, 33, 2, 64), (2, 0, 2, 64), (2, 33, 0, 64), (2, 33, 2, 72), (2, 33, 2, 40), (65536, 33, 65536, 64), (1, 33, 1 << 24, 64)]


def _refused(rc, name):
    from dmvae_amd._lib import DmvaeHipError
    _, ops = _api()
    with pytest.raises(DmvaeHipError):
        ops.check(rc, name)


def _heads_calls_refuse(b, s, h, d, qd, scale, null=None):
    L, ops = _api()
    g = torch.Generator().manual_seed(7)
    mk = lambda *sh: torch.randn(*sh, generator=g).to(BF).to(DEV)
    q, k, v, o, do, lse = mk(4, 33, 96), mk(4, 33, 96), mk(4, 33, 72), mk(2, 33, 144), mk(2, 33, 144), torch.zeros(4, 33, device=DEV)
    out, lo = Out(o.shape, BF), Out(lse.shape, F32)
    dq, dk, dv, delta = Out(q.shape, BF), Out(k.shape, BF), Out(v.shape, BF), Out(lse.shape, F32)
    p = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), do=do.data_ptr(), lse=lse.data_ptr(), out=out.ptr(), lo=lo.ptr(), dq=dq.ptr(), dk=dk.ptr(),
             dv=dv.ptr(), delta=delta.ptr())
    if null:
        p[null] = None
    if null in (None, "q", "k", "v", "out"):
        _refused(L.dmvae_attention_heads_stream_bf16(p["q"], p["k"], p["v"], p["out"], p["lo"], b, s, h, d, qd, scale, ops._stream()), "attention_heads_stream_bf16")
    if null != "out":
        _refused(L.dmvae_attention_bwd_heads_stream_bf16(p["q"], p["k"], p["v"], p["o"], p["do"], p["lse"], p["dq"], p["dk"], p["dv"], p["delta"], b, s, h, d, qd, scale,
                                                         ops._stream()), "attention_bwd_heads_stream_bf16")
    torch.cuda.synchronize()
    for t in (out, lo, dq, dk, dv, delta):
        t.untouched("heads %r scale %r null %r" % ((b, s, h, d, qd), scale, null))


def _packed_calls_refuse(b, s, h, d, scale, null=None):
    L, ops = _api()
    g = torch.Generator().manual_seed(8)
    mk = lambda *sh: torch.randn(*sh, generator=g).to(BF).to(DEV)
    qkv, o, do, lse = mk(2, 33, 3 * 2 * 72), mk(2, 33, 144), mk(2, 33, 144), torch.zeros(4, 33, device=DEV)
    out, lo, dqkv, delta = Out(o.shape, BF), Out(lse.shape, F32), Out(qkv.shape, BF), Out(lse.shape, F32)
    p = dict(qkv=qkv.data_ptr(), o=o.data_ptr(), do=do.data_ptr(), lse=lse.data_ptr(), out=out.ptr(), lo=lo.ptr(), dqkv=dqkv.ptr(), delta=delta.ptr())
    if null:
        p[null] = None
    if null in (None, "qkv", "out"):
        _refused(L.dmvae_attention_qkv_stream_bf16(p["qkv"], p["out"], p["lo"], b, s, h, d, scale, ops._stream()), "attention_qkv_stream_bf16")
    if null != "out":
        _refused(L.dmvae_attention_bwd_qkv_stream_bf16(p["qkv"], p["o"], p["do"], p["lse"], p["dqkv"], p["delta"], b, s, h, d, scale, ops._stream()), "attention_bwd_qkv_stream_bf16")
    torch.cuda.synchronize()
    for t in (out, lo, dqkv, delta):
        t.untouched("packed %r scale %r null %r" % ((b, s, h, d), scale, null))


@pytest.mark.parametrize("b,s,h,d,qd", BAD_HEADS_SHAPES)
def test_heads_entries_refuse_shapes(b, s, h, d, qd):
    _heads_calls_refuse(b, s, h, d, qd, 0.125)


@pytest.mark.parametrize("scale", BAD_SCALES)
def test_heads_entries_refuse_scale(scale):
    _heads_calls_refuse(2, 33, 2, 72, 96, scale)


@pytest.mark.parametrize("null", ["q", "k", "v", "out", "o", "do", "lse", "dq", "dk", "dv", "delta"])
def test_heads_entries_refuse_null_operands(null):
    _heads_calls_refuse(2, 33, 2, 72, 96, 72 ** -0.5, null)


@pytest.mark.parametrize("b,s,h,d", BAD_PACKED_SHAPES)
def test_packed_entries_refuse_shapes(b, s, h, d):
    _packed_calls_refuse(b, s, h, d, 0.125)


@pytest.mark.parametrize("scale", BAD_SCALES)
def test_packed_entries_refuse_scale(scale):
    _packed_calls_refuse(2, 33, 2, 64, scale)


@pytest.mark.parametrize("null", ["qkv", "out", "o", "do", "lse", "dqkv", "delta"])
def test_packed_entries_refuse_null_operands(null):
    _packed_calls_refuse(2, 33, 2, 64, 0.125, null)
