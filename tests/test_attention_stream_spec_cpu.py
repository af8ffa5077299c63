"""The streaming half of tests/attention_spec.py without a GPU: every input class against its purpose at every token count it is used at, the f32 / bf16
emulations of csrc/attention_stream.hip and csrc/attention_bwd_stream.hip (in kernel order) inside every streaming bar on every shared case, and the negative
controls -- one-line mutants of the emulations that have to leave a named bar on a named case.  The emulations are the only arbiter of the bars' width.

Shared cases: head dims 64 and 72 (dq / dk rows of 96) x STREAM_TOKENS (1 .. 577: every count at which a mechanism changes) x randn, negative, ascending, last,
all ten classes at 257 (one live key in the last tile), 289 (ragged) and 320 (whole tiles), and 1025 tokens once per head dim.  The backward emulation runs twice per
case: on the forward emulation's own out / lse, and on bf16(o) / f32(lse) of the definition.

Worst |error| / bound of the emulations (test_emulations_stay_inside_every_streaming_bar prints them; the condition is < 1): out 0.726, lse 0.063; own operands dq 0.243,
dk 0.295, dv 0.834, delta 0.170; made operands dq 0.433, dk 0.529, dv 0.886, delta 0.353.  No site was missing: no term was added after the first run.
Class conditions (test_the_maximum_travels_as_the_class_says, d 64 / 72 x 65 .. 1025 tokens x three seeds): ascending smallest gap 0.811, largest score 16.03;
descending 0.812 and 16.01.

Negative controls (test_negative_controls prints every ratio): |error| / bound of each one-line mutant on the cases it is named for --
  leak (one padded key of the last tile unmasked)           lse 25 on randn S 289, 7.8 at 577, 4.4 at 1025 (out stays at 0.55 / 0.44 / 0.47); out 67 on negative S 289,
                                                            92 on negative S 97 d 72
  alpha_o_only (factor on the accumulators, not on l)       lse 3.4e4 on ascending S 289, 4.0e4 on randn; descending (every later factor 1) is the unchanged kernel
  alpha_l_only (factor on l, not on the accumulators)       out 476 on ascending S 289, 3.2e3 on randn; lse stays inside (0.02)
  alpha_sign (sign of the difference reversed)              out 141, lse 1.8e5 on ascending S 289; out 333 on ascending S 129 d 72
  half_max (running maximum from the lane's own half)       lse 2.2e5 on spike S 289, 1.1e4 on spike_last S 289, 1.5e5 on spike_last S 320 d 72; also randn (lse 3.8e4)
  l_rounded (l from the bf16-rounded p)                     lse 11 on randn S 289, 15 at S 65; out stays inside (0.49); zeroq (p = 1 exactly) cannot show it
  lse_half (lse from one half's sum)                        lse 4.4e4 on randn S 289, 5.5e4 on zeroq S 257 d 72
  stale_block (second block reads the previous tile)        out 400 on randn S 289, 44 on ascending S 129 d 72, 833 on last S 97
  skip_one_q (query pass skips a block of ONE live key)     dq 22 on randn S 97; `last` S 97 cannot show it (dS of the dominant key is ~0: dq 0.02 with and without)
  skip_one_k (key pass, the same)                           dv 93, dk 7.9 on randn S 97; dv 8.8, dk 1.2 on last S 97; dv 11 on last S 97 d 72
  kpass_256 (96-wide key pass on a 256-key grid)            dk, dv infinite at S 129 d 72: keys 128 .. are nobody's and the NaN pre-fill stays
  p_from_max (P from the running maximum, not L)            dv 1.2e3, dq 417 on randn S 289; dq 3.5e3 on zeroq S 320 d 72; `last` (log l ~ 0) cannot show it
  pad_cols (non-zero padded columns 72 .. 95 of dq / dk)    not a bar: the exact-zero condition fails
  delta_unrounded_o                                         NOT told: delta 0.056 at worst (see UNTOLD)
  ds_round_first                                            NOT told: dq 0.24, dk 0.31 at worst (see UNTOLD)
The gap this closes (test_leaked_key_is_caught_where_the_whole_tensor_bars_were_blind, randn at d 64): with the leak the old forward bars see out max err 8e-3 of a bar
of 7.2e-2, rel-L2 1.9e-3 of 6e-3 and an lse error of 1.1e-3 / 4.6e-4 / 3.1e-4 of 2e-3 at 289 / 577 / 1025 tokens -- all pass -- where the streaming lse bar is left
25 / 7.8 / 4.4 times over.
"""
import pytest
import torch

import attention_spec as A

B, H = 1, 2
DIMS = [64, 72]
ONCE = [("randn", 1025, 64), ("ascending", 1025, 72)]      # 1025 tokens once per head dim


def _shared_cases():
    return [(kind, s, d) for d in DIMS for s in A.STREAM_TOKENS for kind in A.stream_classes_at(s)] + ONCE


def _all(c, operands="kernel"):
    ref = A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"])
    fwd = A.bars_forward_stream(c["q"], c["k"], c["v"], c["scale"], ref)
    return ref, fwd, A.bars_backward_stream(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd, operands)


# ---- the classes ----------------------------------------------------------------------------------------------------------------------------
def test_every_class_does_what_it_is_for_at_streaming_token_counts():
    for kind, s, d in _shared_cases():
        c = A.make_case(kind, B, H, s, d)
        A.check_class(c, A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"]))


@pytest.mark.parametrize("kind", ["ascending", "descending"])
def test_the_maximum_travels_as_the_class_says(kind):
    """the issue's own sweep: both head dims, every token count above one tile, three seeds; prints the smallest gap and the largest score"""
    gap, top = float("inf"), 0.0
    for d in DIMS:
        for s in (65, 96, 97, 127, 128, 129, 255, 256, 257, 289, 320, 321, 513, 577, 1025):
            for seed in range(3):
                c = A.make_case(kind, 1, 1, s, d, seed=seed)
                x = A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"])["x"]
                A.check_class(c, dict(x=x))
                tm = A.tile_max(x)
                g = (tm[..., 1:] - torch.cummax(tm, -1).values[..., :-1]) if kind == "ascending" else (tm[..., :1] - tm[..., 1:])
                gap, top = min(gap, float(g.min())), max(top, float(x.max()))
    print("[fig] %s: smallest gap %.3f, largest score %.3f" % (kind, gap, top))
    assert gap >= 0.5 and top <= 16.1


def test_the_last_key_of_the_last_tile_carries_the_spike():
    for s in (65, 257, 289, 320):
        c = A.make_case("spike_last", B, H, s, 64)
        assert float(c["k"][:, s - 1].float().norm(dim=-1).min()) > 50 and float(c["k"][:, :s - 1].float().norm(dim=-1).max()) < 0.1


# ---- the emulations inside the bars ---------------------------------------------------------------------------------------------------------------
def _hold_case(c, tag, rows=None):
    """forward, then the backward twice: on the forward emulation's own out / lse (bars with the forward's terms) and on bf16(o), f32(lse) of the definition"""
    ref, fwd, bwd = _all(c)
    out, lse, _ = A.emulate_forward_stream(c["q"], c["k"], c["v"], c["scale"])
    A.hold(out, ref["o"], fwd["o"], tag + " out", "out")
    A.hold(lse, ref["lse"], fwd["lse"], tag + " lse", "lse")
    bwd_r = A.bars_backward_stream(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd, "reference")
    o_r, lse_r = A.reference_operands(ref)
    d = c["d"]
    for form, o_, l_, bars in (("own", out, lse, bwd), ("reference", o_r, lse_r, bwd_r)):
        dq, dk, dv, delta = A.emulate_backward_stream(c["q"], c["k"], c["v"], o_, c["do"], l_, c["scale"], rows=rows)
        assert A.padded_columns_are_zero(dq, d) and A.padded_columns_are_zero(dk, d)
        for n, g in (("dq", dq[..., :d]), ("dk", dk[..., :d]), ("dv", dv)):
            A.hold(g, ref[n], bars[n], "%s %s (%s)" % (tag, n, form), "%s (%s operands)" % (n, form))
        A.hold(delta, ref["delta"].squeeze(-1), bars["delta"], "%s delta (%s)" % (tag, form), "delta (%s operands)" % form)


def test_emulations_stay_inside_every_streaming_bar():
    A.FIG.clear()
    for kind, s, d in _shared_cases():
        _hold_case(A.make_case(kind, B, H, s, d), "%s S %d d %d" % (kind, s, d), rows=96 if d == 72 else None)
    for k, v in A.FIG.items():
        print("[fig] %s: worst emulation |err| / bound %.3f (bar 1)" % (k, v))
    assert A.FIG and max(A.FIG.values()) < 1.0


# ---- negative controls ----------------------------------------------------------------------------------------------------------------------
# name -> [(class, S, d, the bar it has to leave on that case, or None: printed only)].  Each is one changed line of an emulation (attention_spec: `mutant`).
CONTROLS = {
    "leak": [("randn", 289, 64, "lse"), ("negative", 289, 64, "out"), ("negative", 97, 72, "out"), ("randn", 577, 64, "lse"), ("randn", 1025, 64, "lse")],
    "alpha_o_only": [("ascending", 289, 64, "lse"), ("randn", 289, 64, "lse"), ("descending", 289, 64, None)],
    "alpha_l_only": [("ascending", 289, 64, "out"), ("randn", 289, 64, "out"), ("descending", 289, 64, None)],
    "alpha_sign": [("ascending", 289, 64, "out"), ("ascending", 129, 72, "lse"), ("descending", 289, 64, None)],
    "half_max": [("spike", 289, 64, "lse"), ("spike_last", 289, 64, "lse"), ("spike_last", 320, 72, "lse"), ("randn", 289, 64, None)],
    "l_rounded": [("randn", 289, 64, "lse"), ("randn", 65, 64, "lse"), ("zeroq", 320, 72, None)],
    "lse_half": [("randn", 289, 64, "lse"), ("zeroq", 257, 72, "lse")],
    "stale_block": [("randn", 289, 64, "out"), ("ascending", 129, 72, "out"), ("last", 97, 64, "out")],
    "skip_one_q": [("randn", 97, 64, "dq"), ("randn", 97, 72, "dq"), ("negative", 97, 72, None), ("last", 97, 64, None)],
    "skip_one_k": [("last", 97, 64, "dk"), ("randn", 97, 64, "dv"), ("last", 97, 72, "dv")],
    "kpass_256": [("randn", 129, 72, "dk"), ("randn", 129, 72, "dv")],
    "p_from_max": [("randn", 289, 64, "dv"), ("zeroq", 320, 72, "dq"), ("last", 97, 64, None)],
    "delta_unrounded_o": [("randn", 289, 64, "delta"), ("randn4", 289, 64, "delta"), ("offset", 320, 72, "delta")],
    "ds_round_first": [("randn", 289, 72, "dq"), ("randn4", 257, 72, "dk"), ("randn", 97, 64, "dq")],
    "pad_cols": [("randn", 97, 72, "pad"), ("randn", 289, 72, "pad")],
}
# Controls the bars cannot tell from the kernel's order, with the reason; test_negative_controls prints the measured worst ratio next to each.
#   delta_unrounded_o  delta from the f32 O is CLOSER to the definition than the kernel's: the bar has to admit the stored O's bf16 rounding, so a delta without it
#                      sits well inside (0.06 to 0.09 of the bar).  What the bars cannot see here is a backward that is more exact than its operands allow.
#   ds_round_first     as in the resident work: a second bf16 rounding of dS doubles one site's half-ulp per element, which the bar takes at its worst-case sum over
#                      the keys while the errors add up like a random walk.
UNTOLD = {"delta_unrounded_o", "ds_round_first"}


def _control_ratios(name, kind, s, d):
    c = A.make_case(kind, B, H, s, d)
    ref, fwd, bwd = _all(c)
    if name in A.FORWARD_STREAM_MUTANTS:
        out, lse, _ = A.emulate_forward_stream(c["q"], c["k"], c["v"], c["scale"], mutant=name)
        return {"out": A.ratio(out, ref["o"], fwd["o"]), "lse": A.ratio(lse, ref["lse"], fwd["lse"])}
    out, lse, x = A.emulate_forward_stream(c["q"], c["k"], c["v"], c["scale"])
    dq, dk, dv, delta = A.emulate_backward_stream(c["q"], c["k"], c["v"], out, c["do"], lse, c["scale"], rows=96 if d == 72 else None, mutant=name, o32=x["o32"], m=x["m"])
    r = {n: A.ratio(g, ref[n], bwd[n]) for n, g in (("dq", dq[..., :d]), ("dk", dk[..., :d]), ("dv", dv))}
    r["delta"] = A.ratio(delta, ref["delta"].squeeze(-1), bwd["delta"])
    r["pad"] = 0.0 if A.padded_columns_are_zero(dq, d) and A.padded_columns_are_zero(dk, d) else float("inf")      # not a bar: exact zeros or not
    return r


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_negative_controls(name):
    assert name in A.FORWARD_STREAM_MUTANTS + A.BACKWARD_STREAM_MUTANTS
    worst = 0.0
    for kind, s, d, bar in CONTROLS[name]:
        r = _control_ratios(name, kind, s, d)
        print("[control] %s on %s S %d d %d (names %s): %s" % (name, kind, s, d, bar, ", ".join("%s %.3g" % kv for kv in r.items())))
        if bar is None:
            continue
        worst = max(worst, r[bar])
        if name not in UNTOLD:
            assert r[bar] > 1.0, "%s stays inside the %s bar on %s S %d d %d (ratio %.3g)" % (name, bar, kind, s, d, r[bar])
    if name in UNTOLD:
        print("[control] %s: NOT told from the kernel's order by the bars, worst ratio %.3g (see UNTOLD)" % (name, worst))
        assert worst <= 1.0, "the bars do tell %s: take it out of UNTOLD" % name


def test_mutant_lists_are_all_controlled():
    assert sorted(CONTROLS) == sorted(A.FORWARD_STREAM_MUTANTS + A.BACKWARD_STREAM_MUTANTS)


@pytest.mark.parametrize("s", [289, 577, 1025])
def test_leaked_key_is_caught_where_the_whole_tensor_bars_were_blind(s):
    """randn x 1.5, one padded key of the last tile unmasked: the old forward bars (max|err| < 2e-2 max|ref| + 1e-3, rel-L2 < 6e-3, |lse err| < 2e-3) pass, the
    per-element lse bar does not"""
    c = A.make_case("randn", 1, 2, s, 64)
    ref, fwd, _ = _all(c)
    out, lse, _ = A.emulate_forward_stream(c["q"], c["k"], c["v"], c["scale"], mutant="leak")
    oerr = float((out.double() - ref["o"]).abs().max())
    obar = 2e-2 * float(ref["o"].abs().max()) + 1e-3
    rl2 = float((out.double() - ref["o"]).norm() / ref["o"].norm())
    lerr = float((lse.double() - ref["lse"]).abs().max())
    r_out, r_lse = A.ratio(out, ref["o"], fwd["o"]), A.ratio(lse, ref["lse"], fwd["lse"])
    print("[control] leak on randn S %d: out max err %.2g (old bar %.2g), rel-L2 %.2g (old bar 6e-3), lse err %.2g (old bar 2e-3); streaming bars: out %.3g, lse %.3g"
          % (s, oerr, obar, rl2, lerr, r_out, r_lse))
    assert oerr < obar and rl2 < 6e-3 and lerr < 2e-3
    assert r_lse > 1.0
