"""The d = 512 streaming attention kernels (csrc/attention_wide.hip, csrc/attention_wide_bwd.hip; one head, any S) through their two C entries, against the fp64
definition and the per-element wide bars of tests/attention_spec.py (-m gpu).  The references run on the GPU in torch double.  Every output -- out, lse, dq, dk, dv
and delta -- is carved out of a buffer with a 4096-byte guard zone on BOTH sides and pre-filled with 0xFF bytes (NaN in bf16 and f32): the guards must come back
untouched, no NaN may survive in the live region, and every element is held to its bar.  The backward runs twice per case: on the forward kernel's own lse (the
pipeline; bars with the forward's terms) and on f32(lse) of the definition, so that a forward defect can neither hide nor cause a backward failure.

Bit identities: a rerun; the forward with and without lse; the backward with `o` replaced by a buffer of 0xFF bytes (the header's "not read"); B = 3 at S = 65 against
three B = 1 calls; 104 samples at S = 289 (520 forward and 1040 backward workgroups behind xcd_remap: more than one round of CUs, every remap class) against calls of
8 samples.  Refusals return non-zero, leave a message that names the entry, and write nothing.

Which kernels a case launches: forward attention_wide_kernel on B ceil(S / 64) workgroups; backward attention_wide_bwd_dq_kernel, then
attention_wide_bwd_dkdv_kernel, each on B ceil(S / 32).

Worst |err| / bound observed on an MI355X (bar 1; over every element of every case of this module), per entry and output:
  dmvae_attention_wide_stream_bf16        out 0.491, lse 0.042
  dmvae_attention_wide_bwd_stream_bf16    own lse   dq 0.846, dk 0.698, dv 0.646, delta 0.013
                                          made lse  dq 0.848, dk 0.869, dv 0.751, delta 0.021
The CPU emulations of tests/test_attention_wide_spec_cpu.py reach out 0.612, lse 0.022; own lse dq 0.826, dk 0.687, dv 0.660, delta 0.012; made lse dq 0.829,
dk 0.869, dv 0.750, delta 0.030: the kernels sit where their emulations do.  The negative controls (every one told, two inert padded-row mutants) are listed in that
module's docstring.  Every bit identity above held, every refusal returned an error with nothing written, and no test found a kernel at fault.  The whole module runs
in a few seconds.
"""
import pytest
import torch

import attention_spec as A
from attention_spec import BF, F32
from test_gpu_attention_stream_spec import DEV, Out, figs  # noqa: F401  (the guard-zone outputs and the figure printer of the streaming module)

pytestmark = pytest.mark.gpu
C = A.WIDE_D
FWD, BWD = "dmvae_attention_wide_stream_bf16", "dmvae_attention_wide_bwd_stream_bf16"


def _api():
    from dmvae_amd import _lib, ops
    return _lib.lib(), ops


# ---- the two entries, outputs allocated here ---------------------------------------------------------------------------------------------------------
def wide_fwd(q, k, v, scale, what, want_lse=True):
    """q, k, v [B, S, 512] -> (out [B, S, 512], lse [B, S] or None)"""
    L, ops = _api()
    b, s, _ = q.shape
    out, lse = Out((b, s, C), BF), Out((b, s), F32) if want_lse else None
    ops.check(L.dmvae_attention_wide_stream_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.ptr(), lse.ptr() if lse else None, b, s, C, float(scale), ops._stream()), FWD)
    return out.ok(what + " out"), lse.ok(what + " lse") if lse else None


def wide_bwd(q, k, v, o, do, lse, scale, what):
    """-> dq, dk, dv [B, S, 512], delta [B, S]"""
    L, ops = _api()
    b, s, _ = q.shape
    dq, dk, dv, delta = Out((b, s, C), BF), Out((b, s, C), BF), Out((b, s, C), BF), Out((b, s), F32)
    ops.check(L.dmvae_attention_wide_bwd_stream_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.ptr(), dk.ptr(), dv.ptr(),
                                                     delta.ptr(), b, s, C, float(scale), ops._stream()), BWD)
    return dq.ok(what + " dq"), dk.ok(what + " dk"), dv.ok(what + " dv"), delta.ok(what + " delta")


def _bars(c):
    ref = A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"])
    fwd = A.bars_forward_wide(c["q"], c["k"], c["v"], c["scale"], ref)
    own = A.bars_backward_wide(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd, "kernel")
    made = A.bars_backward_wide(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd, "reference")
    return ref, fwd, own, made


def _hold_grads(got, ref, bars, what, form):
    for n, g in zip(("dq", "dk", "dv"), got[:3]):
        A.hold(g, ref[n], bars[n], "%s %s" % (what, n), "%s %s (%s lse)" % (BWD, n, form))
    A.hold(got[3], ref["delta"].squeeze(-1), bars["delta"], what + " delta", "%s delta (%s lse)" % (BWD, form))


def _same(x, y):
    return all(torch.equal(a, b) for a, b in zip(x, y))


def _sub(c, sl):
    cc = {n: c[n][sl].contiguous() for n in ("q", "k", "v", "do")}
    cc.update(scale=c["scale"])
    return cc


# ---- every token count: every element of all six outputs, and the bit identities that need no second shape --------------------------------------------------
@pytest.mark.parametrize("s", A.WIDE_TOKENS)
def test_every_element_at_every_token_count(s, figs):
    for kind in A.wide_classes_at(s):
        c = A.to_dev(A.make_wide_case(kind, s, seed=1), DEV)
        what = "%s S %d" % (kind, s)
        ref, fwd, own, made = _bars(c)
        A.check_class(c, ref)
        q, k, v, do, scale = c["q"], c["k"], c["v"], c["do"], c["scale"]
        out, lse = wide_fwd(q, k, v, scale, what)
        A.hold(out, ref["o"], fwd["o"], what + " out", FWD + " out")
        A.hold(lse, ref["lse"], fwd["lse"], what + " lse", FWD + " lse")
        out_n, _ = wide_fwd(q, k, v, scale, what + " no lse", want_lse=False)
        assert torch.equal(out, out_n), what + ": the forward without lse gives other bits"
        g_own = wide_bwd(q, k, v, out, do, lse, scale, what + " own lse")
        _hold_grads(g_own, ref, own, what + " (own lse)", "own")
        o_r, l_r = A.reference_operands(ref)
        g_made = wide_bwd(q, k, v, o_r, do, l_r.contiguous(), scale, what + " made lse")
        _hold_grads(g_made, ref, made, what + " (made lse)", "made")
        out2, lse2 = wide_fwd(q, k, v, scale, what + " rerun")
        assert torch.equal(out, out2) and torch.equal(lse, lse2), what + ": forward rerun differs"
        assert _same(g_own, wide_bwd(q, k, v, out, do, lse, scale, what + " rerun")), what + ": backward rerun differs"
        junk = torch.full_like(out.view(torch.int16), -1).view(BF)      # 0xFF bytes: NaN in every channel
        assert _same(g_own, wide_bwd(q, k, v, junk, do, lse, scale, what + " o of 0xFF")), what + ": the backward read `o`"


def test_a_3b_call_equals_three_b_calls():
    b, s = 3, 65
    c = A.to_dev(A.make_wide_case("randn", s, b=b, seed=4), DEV)
    out, lse = wide_fwd(c["q"], c["k"], c["v"], c["scale"], "3B")
    g = wide_bwd(c["q"], c["k"], c["v"], out, c["do"], lse, c["scale"], "3B")
    for i in range(b):
        cc = _sub(c, slice(i, i + 1))
        o_c, l_c = wide_fwd(cc["q"], cc["k"], cc["v"], cc["scale"], "B")
        assert torch.equal(out[i:i + 1], o_c) and torch.equal(lse[i:i + 1], l_c), "forward of sample %d differs from its own call" % i
        assert _same([t[i:i + 1] for t in g], wide_bwd(cc["q"], cc["k"], cc["v"], o_c, cc["do"], l_c, cc["scale"], "B")), "backward of sample %d differs" % i


def test_many_blocks(figs):
    """104 samples at 289 tokens: 520 forward and 1040 backward workgroups, more than one round of CUs and every xcd_remap class.  spread_items against fp64; EVERY
    sample bit for bit against the same samples run 8 at a time -- with the NaN pre-fill and the guards, every (sample, block) behind xcd_remap is computed, in place."""
    b, s, step = 104, 289, 8
    c = A.to_dev(A.make_wide_case("randn", s, b=b, seed=2), DEV)
    what = "%d samples S %d" % (b, s)
    items = torch.tensor(A.spread_items(b), device=DEV)
    ref, fwd, own, _ = _bars(_sub(c, items))
    out, lse = wide_fwd(c["q"], c["k"], c["v"], c["scale"], what)
    A.hold(out[items], ref["o"], fwd["o"], what + " out", FWD + " out")
    A.hold(lse[items], ref["lse"], fwd["lse"], what + " lse", FWD + " lse")
    g = wide_bwd(c["q"], c["k"], c["v"], out, c["do"], lse, c["scale"], what)
    _hold_grads([t[items] for t in g], ref, own, what + " (own lse)", "own")
    for b0 in range(0, b, step):
        sl = slice(b0, b0 + step)
        cc = _sub(c, sl)
        o_c, l_c = wide_fwd(cc["q"], cc["k"], cc["v"], cc["scale"], what + " chunk")
        assert torch.equal(out[sl], o_c) and torch.equal(lse[sl], l_c), what + ": forward of samples %d.. differs from the small call" % b0
        assert _same([t[sl] for t in g], wide_bwd(cc["q"], cc["k"], cc["v"], o_c, cc["do"], l_c, cc["scale"], what + " chunk")), \
            what + ": backward of samples %d.. differs from the small call" % b0


# ---- refusals: an error code before any launch, a message, nothing written ------------------------------------------------------------------------------
BAD_SCALES = [0.0, -0.125, float("inf"), float("-inf"), float("nan")]
BAD_SHAPES = [(2, 33, 256), (2, 33, 511), (2, 33, 576), (2, 33, 64), (2, 33, 0), (2, 0, 512), (0, 33, 512), (-1, 33, 512), (2, -5, 512)]      # (batch, seq, channels)


def _calls_refuse(b, s, ch, scale, null=None):
    """the operands are those of a valid 2 x 33 x 512 call; both entries (the forward only where the changed argument is one of its own) must refuse"""
    L, ops = _api()
    g = torch.Generator().manual_seed(7)
    mk = lambda: torch.randn(2, 33, C, generator=g).to(BF).to(DEV)
    q, k, v, o, do, lse = mk(), mk(), mk(), mk(), mk(), torch.zeros(2, 33, device=DEV)
    out, lo = Out((2, 33, C), BF), Out((2, 33), F32)
    dq, dk, dv, delta = Out((2, 33, C), BF), Out((2, 33, C), BF), Out((2, 33, C), BF), Out((2, 33), F32)
    p = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), do=do.data_ptr(), lse=lse.data_ptr(), out=out.ptr(), lo=lo.ptr(), dq=dq.ptr(), dk=dk.ptr(),
             dv=dv.ptr(), delta=delta.ptr())
    if null:
        p[null] = None
    calls = []
    if null in (None, "q", "k", "v", "out"):
        calls.append((FWD, lambda: L.dmvae_attention_wide_stream_bf16(p["q"], p["k"], p["v"], p["out"], p["lo"], b, s, ch, scale, ops._stream())))
    if null != "out":
        calls.append((BWD, lambda: L.dmvae_attention_wide_bwd_stream_bf16(p["q"], p["k"], p["v"], p["o"], p["do"], p["lse"], p["dq"], p["dk"], p["dv"], p["delta"], b, s, ch,
                                                                       scale, ops._stream())))
    tag = "%r scale %r null %r" % ((b, s, ch), scale, null)
    for name, call in calls:
        rc = call()
        assert rc != 0, "%s accepted %s" % (name, tag)
        msg = (L.dmvae_last_error() or b"").decode()
        assert name[len("dmvae_"):] in msg, "%s refused %s without naming itself in the error: %r" % (name, tag, msg)
        with pytest.raises(_lib_error()):
            ops.check(rc, name)
    torch.cuda.synchronize()
    for t in (out, lo, dq, dk, dv, delta):
        t.untouched(tag)


def _lib_error():
    from dmvae_amd._lib import DmvaeHipError
    return DmvaeHipError


@pytest.mark.parametrize("b,s,ch", BAD_SHAPES)
def test_entries_refuse_shapes(b, s, ch):
    _calls_refuse(b, s, ch, C ** -0.5)


@pytest.mark.parametrize("scale", BAD_SCALES)
def test_entries_refuse_scale(scale):
    _calls_refuse(2, 33, C, scale)


@pytest.mark.parametrize("null", ["q", "k", "v", "out", "o", "do", "lse", "dq", "dk", "dv", "delta"])
def test_entries_refuse_null_operands(null):
    _calls_refuse(2, 33, C, C ** -0.5, null)
