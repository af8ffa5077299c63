"""The d = 512 third of tests/attention_spec.py without a GPU: the reference pieces against fp64 autograd, every input class against its purpose over 32-key tiles,
the f32 / bf16 emulations of csrc/attention_wide.hip and csrc/attention_wide_bwd.hip (in kernel order) inside every wide bar on every shared case, and the negative
controls -- one-line mutants of the emulations that have to leave a named bar on a named case.  The emulations are the only arbiter of the bars' width.

Shared cases: make_case(kind, 1, 1, S, 512, tile=32) x WIDE_TOKENS (1 .. 1296) x randn, negative, ascending, last, and all ten classes at 33, 97 and 1025 tokens
(one live key in the last tile).  The backward emulation runs twice per case: on the forward emulation's own lse, and on f32(lse) of the definition.

Worst |error| / bound of the emulations (test_emulations_stay_inside_every_wide_bar prints them; the condition is < 1): out 0.612, lse 0.022; own lse dq 0.826,
dk 0.687, dv 0.660, delta 0.012; made lse dq 0.829, dk 0.869, dv 0.750, delta 0.030.  No site was missing: no term was added after the first run.
Class conditions over 32-key tiles (test_the_maximum_travels_over_32_key_tiles, 33 .. 1296 tokens x three seeds): ascending smallest gap 0.338 (0.99 of 14 / nt,
nt = 41 at 1296 tokens), largest score 16.00; descending 0.335 and 16.01.

Negative controls (test_negative_controls prints every ratio): |error| / bound of each one-line mutant on the cases it is named for --
  leak (one padded key of the last tile unmasked)            out 108 on negative S 33, 89 at S 97; lse 3.0e4 on offset S 97, 16 on randn S 33, 26 on zeroq S 1025.
                                                             randn S 1025 does NOT show it (lse 0.17, out 0.38; printed): see the last paragraph
  mask_ignores_half (lim without the 4 kg)                   the upper half-wave lets ONE padded key through at S = 17, 33, 97, 1025 (key 32 t + lim + 3): leak's
                                                             figures (out 117 on negative S 17)
  alpha_o_only (factor on the accumulators, not on l)        lse 9.6e3 on ascending S 97, 1.5e4 on last S 1296; out 113 on last S 97
  alpha_l_only (factor on l, not on the accumulators)        out 1.2e6 on last S 97, 1.3e7 on randn4 S 1025; lse stays inside (0.04)
  half_max (running maximum from the lane's own half)        lse 3.1e4 on spike S 33 / 97, 3.0e4 at S 1025; out 4.4e6 on randn4 S 1025
  lse_half (lse from one half's sum)                         lse 1.8e5 on zeroq S 33, infinite on spike (the half without the spike sums to 0); out is untouched
  l_rounded (l from the bf16-rounded p)                      lse 2.5 on negative S 33, 2.4 at S 65; out stays inside (0.57)
  stale_tile (K / V image of tile t - 1)                     out 1.7e5 on randn4 S 97, 3.9e4 on last S 97; lse 3.1e4 on spike_last S 33
  delta_from_O (dO . O on the bf16 O, the sibling's site)    delta 33 (own lse) / 40 (made) on last S 1025, 26 on ascending S 33; dq 19 / 21 on last S 1025
  ds_single_bf16 (lo dropped)                                dq 3.9 on zeroq S 33, 3.5 on randn S 97 (made); dk 2.7 on last S 33 (made), 3.1 on randn S 17 (made)
  quarter_dropped (the fourth wave's partial block)          every output: dq 1.1e20, delta 7.0e10 on offset S 1025; dq 716, dk 671, dv 861, delta 921 on randn S 97
  p_from_max (P from the running maximum, not L)             dq 2.8e7, dv 2.5e4 on zeroq S 1025; dk 7.7e4 on negative S 1296
  dk_noscale                                                 dk 4.8e3 on last S 33 and randn S 33; dq, dv, delta untouched
  skip_one_q (query pass: the single live key at 32 k + 1)   delta 6.2e3 on last S 33, dq 1.0e3 on zeroq S 33, 475 on randn S 97
  skip_one_k (key pass: the single live query at 32 k + 1)   dv 105, dk 387 on randn S 33; dk 301 on randn S 1025
Every control is told; none is recorded as "not told".
INERT, neither told nor not told (test_padded_row_mutants_are_inert): pad_key_unselected and pad_query_finite_L.  A padded K, V, Q or dO row is staged as zeros.
  pad_key_unselected   a padded key keeps p = exp(0 - L) instead of 0.  In the first walk it adds fmaf(p, dP, delta) with dP = dO . 0 = 0: delta's bits stand.  In the
                       second its hi and lo multiply a zero K row: +-0 into dQ.  p is finite for L > -88 (every class: L >= -16), so no 0 * inf.
  pad_query_finite_L   a padded query travels with L and delta of row S - 1 instead of +inf and 0: its p is finite, P^T dO and dS^T Q meet zero dO / Q rows: +-0
                       into dV and dK.  The outputs are bit-identical to the unchanged emulation on every case tried -- asserted, not a ratio.
The gap this closes (test_leaked_key_is_caught_where_the_whole_tensor_bars_were_blind, 1025 tokens): with the leak the old forward bars of
tests/test_gpu_attention_wide.py see, on zeroq, out max err 5.8e-4 of a bar of 4.2e-3, rel-L2 2.0e-3 of 6e-3 and an lse error of 9.8e-4 of 2e-3 -- all pass -- where
the derived lse bar is left 26 times over.  On randn x 1.5 they pass as well (1.1e-2 of 0.13, 1.8e-3, 1.6e-4), and there the derived bars pass TOO (lse 0.17): at 512
channels the scores' own worst-case term, 512 * 2^-24 * scale sum_d |q_d k_d| ~ 1e-3, is as wide as a leak of 1 / 6000 of a row.  That term is a site, not a fit, and
stays; the leak at 1025 tokens is what zeroq (q = 0: the term vanishes), negative and offset are at that count for.
"""
import pytest
import torch

import attention_spec as A


def _shared_cases():
    return [(kind, s) for s in A.WIDE_TOKENS for kind in A.wide_classes_at(s)]


_CACHE = {}


def _all(kind, s):
    """the case, its definition and its three sets of bars; the small ones are kept for the controls that come back to them"""
    if (kind, s) in _CACHE:
        return _CACHE[(kind, s)]
    c = A.make_wide_case(kind, s)
    ref = A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"])
    fwd = A.bars_forward_wide(c["q"], c["k"], c["v"], c["scale"], ref)
    own = A.bars_backward_wide(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd, "kernel")
    made = A.bars_backward_wide(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd, "reference")
    if s <= 200:
        _CACHE[(kind, s)] = (c, ref, fwd, own, made)
    return c, ref, fwd, own, made


# ---- the definition and the classes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,s", [("randn", 33), ("last", 97), ("ascending", 65)])
def test_reference_pieces_against_fp64_autograd(kind, s):
    c = A.make_wide_case(kind, s)
    ref = A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"])
    q, k, v = (c[n].double().clone().requires_grad_(True) for n in ("q", "k", "v"))
    x = c["scale"] * q @ k.transpose(-1, -2)
    o = torch.softmax(x, -1) @ v
    o.backward(c["do"].double())
    lse = torch.logsumexp(x, -1)
    for name, got, want in (("o", ref["o"], o.detach()), ("lse", ref["lse"], lse.detach()), ("dq", ref["dq"], q.grad), ("dk", ref["dk"], k.grad), ("dv", ref["dv"], v.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * (1 + float(want.abs().max())), name
    # delta both ways: sum_k P dP (what the wide kernel forms) and dO . o (what its siblings form) are the same number
    assert float((ref["delta"].squeeze(-1) - (c["do"].double() * ref["o"]).sum(-1)).abs().max()) <= 1e-12 * (1 + float(ref["delta"].abs().max()))
    # sum_k dS = 0: the identity the kernel's own-p delta keeps
    ds = ref["p"] * (ref["dP"] - ref["delta"])
    assert float(ds.sum(-1).abs().max()) <= 1e-12 * float(ds.abs().sum(-1).max() + 1)


def test_every_class_does_what_it_is_for_at_wide_token_counts():
    for kind, s in _shared_cases():
        c = A.make_wide_case(kind, s)
        assert c["tile"] == A.WIDE_TILE and c["d"] == 512 and c["q"].shape == (1, s, 512)
        A.check_class(c, A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"]))


def test_the_tile_parameter_defaults_to_the_streaming_kernels_tiles():
    for kind in ("ascending", "descending", "spike_last", "randn"):
        a, b = A.make_case(kind, 1, 2, 289, 64), A.make_case(kind, 1, 2, 289, 64, tile=A.STREAM_TILE)
        assert all(torch.equal(a[n], b[n]) for n in ("q", "k", "v", "do"))
    a, b = A.make_case("ascending", 1, 1, 289, 512), A.make_wide_case("ascending", 289)
    assert not torch.equal(a["k"], b["k"]) and torch.equal(a["v"], b["v"])


@pytest.mark.parametrize("kind", ["ascending", "descending"])
def test_the_maximum_travels_over_32_key_tiles(kind):
    """every token count above one tile, three seeds; prints the smallest gap between a tile's maximum and the running maximum before it, and the largest score"""
    gap, top, rel = float("inf"), 0.0, float("inf")
    for s in (33, 63, 64, 65, 95, 96, 97, 128, 129, 289, 1025, 1296):
        for seed in range(3):
            c = A.make_wide_case(kind, s, seed=seed)
            x = c["scale"] * c["q"].double() @ c["k"].double().transpose(-1, -2)
            A.check_class(c, dict(x=x))
            tm = A.tile_max(x, A.WIDE_TILE)
            g = (tm[..., 1:] - torch.cummax(tm, -1).values[..., :-1]) if kind == "ascending" else (tm[..., :1] - tm[..., 1:])
            gap, top, rel = min(gap, float(g.min())), max(top, float(x.max())), min(rel, float(g.min()) * A.wide_ntiles(s) / 14)
    print("[fig] %s over 32-key tiles: smallest gap %.3f (%.2f of 14 / nt at worst), largest score %.3f" % (kind, gap, rel, top))
    assert gap >= 0.2 and rel >= 0.6 and top <= 16.1


def test_the_last_key_of_the_last_tile_carries_the_spike():
    for s in (33, 97, 1025):
        c = A.make_wide_case("spike_last", s)
        assert float(c["k"][:, s - 1].float().norm(dim=-1).min()) > 150 and float(c["k"][:, :s - 1].float().norm(dim=-1).max()) < 0.2


# ---- the emulations inside the bars ---------------------------------------------------------------------------------------------------------------
def _run(kind, s, fmut=None, bmut=None):
    """-> ratios: out, lse, and per form ("own": the forward emulation's lse; "made": f32(lse) of the definition) dq, dk, dv, delta; and the raw backward outputs"""
    c, ref, fwd, own, made = _all(kind, s)
    out0, lse0, x0 = A.emulate_forward_wide(c["q"], c["k"], c["v"], c["scale"])
    r, raw = {}, {}
    if bmut is None:
        out, lse, _ = (out0, lse0, x0) if fmut is None else A.emulate_forward_wide(c["q"], c["k"], c["v"], c["scale"], mutant=fmut)
        r["out"], r["lse"] = A.ratio(out, ref["o"], fwd["o"]), A.ratio(lse, ref["lse"], fwd["lse"])
        if fmut is not None:
            return r, raw
    o_r, lse_r = A.reference_operands(ref)
    for form, o_, l_, bars in (("own", out0, lse0, own), ("made", o_r, lse_r, made)):
        g = A.emulate_backward_wide(c["q"], c["k"], c["v"], o_, c["do"], l_, c["scale"], mutant=bmut, m=x0["m"])
        raw[form] = g
        for n, t in zip(("dq", "dk", "dv"), g):
            r["%s (%s lse)" % (n, form)] = A.ratio(t, ref[n], bars[n])
        r["delta (%s lse)" % form] = A.ratio(g[3], ref["delta"].squeeze(-1), bars["delta"])
    return r, raw


def test_emulations_stay_inside_every_wide_bar():
    worst = {}
    for kind, s in _shared_cases():
        r, _ = _run(kind, s)
        for k, v in r.items():
            assert v < 1.0, "%s S %d: the emulation leaves the %s bar (ratio %.3f)" % (kind, s, k, v)
            if v > worst.get(k, (-1.0,))[0]:
                worst[k] = (v, kind, s)
    for k, (v, kind, s) in worst.items():
        print("[fig] %s: worst emulation |err| / bound %.3f (bar 1) on %s S %d" % (k, v, kind, s))
    assert len(worst) == 10


# ---- negative controls ----------------------------------------------------------------------------------------------------------------------
# name -> [(class, S, the bar it has to leave on that case, or None: printed only)].  Each is one changed line of an emulation (attention_spec: `mutant`).
CONTROLS = {
    "leak": [("negative", 33, "out"), ("negative", 97, "out"), ("offset", 97, "lse"), ("zeroq", 1025, "lse"), ("randn", 33, "lse"), ("randn", 1025, None)],
    "mask_ignores_half": [("negative", 17, "out"), ("negative", 33, "out"), ("offset", 97, "lse"), ("zeroq", 1025, "lse"), ("randn", 1025, None)],
    "alpha_o_only": [("ascending", 97, "lse"), ("last", 1296, "lse"), ("last", 97, "out"), ("descending", 97, None)],
    "alpha_l_only": [("last", 97, "out"), ("randn4", 1025, "out"), ("ascending", 65, "out"), ("descending", 97, None)],
    "half_max": [("spike", 33, "lse"), ("spike", 97, "lse"), ("spike", 1025, "lse"), ("randn4", 1025, "out")],
    "lse_half": [("zeroq", 33, "lse"), ("randn", 97, "lse"), ("spike", 97, "lse")],
    "l_rounded": [("negative", 33, "lse"), ("negative", 65, "lse"), ("zeroq", 33, None)],
    "stale_tile": [("randn4", 97, "out"), ("last", 97, "out"), ("spike_last", 33, "lse"), ("randn", 1296, "out")],
    "delta_from_O": [("last", 1025, "delta (own lse)"), ("last", 1025, "delta (made lse)"), ("ascending", 33, "delta (made lse)"), ("last", 1025, "dq (own lse)"),
                     ("randn4", 1025, "dk (made lse)"), ("negative", 97, "delta (own lse)")],
    "ds_single_bf16": [("zeroq", 33, "dq (own lse)"), ("randn", 97, "dq (made lse)"), ("last", 33, "dk (made lse)"), ("randn", 17, "dk (made lse)"),
                       ("negative", 33, "dq (made lse)"), ("ascending", 1296, None)],
    "quarter_dropped": [("offset", 1025, "dq (own lse)"), ("randn", 33, "delta (own lse)"), ("randn", 97, "dv (own lse)"), ("randn", 97, "dk (own lse)")],
    "p_from_max": [("zeroq", 1025, "dq (own lse)"), ("zeroq", 1025, "dv (own lse)"), ("negative", 1296, "dk (own lse)"), ("randn", 97, "delta (made lse)")],
    "dk_noscale": [("last", 33, "dk (own lse)"), ("randn", 33, "dk (made lse)"), ("ascending", 1296, "dk (own lse)")],
    "skip_one_q": [("last", 33, "delta (own lse)"), ("zeroq", 33, "dq (own lse)"), ("randn", 97, "dq (made lse)"), ("randn", 1025, "dq (own lse)")],
    "skip_one_k": [("randn", 33, "dv (own lse)"), ("randn", 33, "dk (made lse)"), ("randn", 1025, "dk (made lse)"), ("last", 97, "dv (own lse)")],
}
INERT = {"pad_key_unselected": [("randn", 33), ("negative", 17), ("last", 97), ("offset", 65), ("randn4", 1025)],
         "pad_query_finite_L": [("randn", 33), ("negative", 17), ("last", 97), ("offset", 65), ("randn4", 1025)]}
UNTOLD = {}          # name -> reason; at most two may stand here.  None does: every control above leaves a bar.


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_negative_controls(name):
    forward = name in A.FORWARD_WIDE_MUTANTS
    assert forward or name in A.BACKWARD_WIDE_MUTANTS
    for kind, s, bar in CONTROLS[name]:
        r, _ = _run(kind, s, fmut=name) if forward else _run(kind, s, bmut=name)
        print("[control] %s on %s S %d (names %s): %s" % (name, kind, s, bar, ", ".join("%s %.3g" % kv for kv in r.items())))
        if bar is not None:
            assert r[bar] > 1.0, "%s stays inside the %s bar on %s S %d (ratio %.3g)" % (name, bar, kind, s, r[bar])


@pytest.mark.parametrize("name", sorted(INERT))
def test_padded_row_mutants_are_inert(name):
    """zero-staged rows: a leaked p of a padded key or query multiplies zeros alone -- the bits of all four outputs are those of the unchanged emulation"""
    for kind, s in INERT[name]:
        assert s % 32, "needs a ragged last tile"
        _, base = _run(kind, s)
        _, mut = _run(kind, s, bmut=name)
        for form in ("own", "made"):
            for n, a, b in zip(("dq", "dk", "dv", "delta"), base[form], mut[form]):
                assert torch.equal(a, b), "%s changes %s on %s S %d (%s lse): not inert" % (name, n, kind, s, form)
    print("[control] %s: inert -- bit-identical outputs on %s" % (name, ", ".join("%s S %d" % ks for ks in INERT[name])))


def test_mutant_lists_are_all_controlled():
    assert sorted(list(CONTROLS) + list(INERT)) == sorted(A.FORWARD_WIDE_MUTANTS + A.BACKWARD_WIDE_MUTANTS)
    assert len(UNTOLD) <= 2 and not set(UNTOLD) & {"leak", "delta_from_O", "ds_single_bf16"}


def test_leaked_key_is_caught_where_the_whole_tensor_bars_were_blind():
    """1025 tokens, one padded key of the last tile unmasked, on zeroq (uniform rows: the leaked key takes 1 / 1026 of every row) and on randn x 1.5: the old
    forward bars of tests/test_gpu_attention_wide.py (max|err| < 2e-2 max|ref| + 1e-3, rel-L2 < 6e-3, |lse err| < 2e-3) pass on both.  The per-element lse bar is left
    on zeroq.  On randn it is NOT: at 512 channels the scores' own worst-case term, 512 * 2^-24 * scale sum_d |q_d k_d| ~ 1e-3, is as wide as the leak (1.7e-4) --
    printed, and the reason the class set has zeroq (q = 0: that term vanishes) at this token count."""
    r_lse = {}
    for kind in ("zeroq", "randn"):
        c, ref, fwd, _, _ = _all(kind, 1025)
        out, lse, _ = A.emulate_forward_wide(c["q"], c["k"], c["v"], c["scale"], mutant="leak")
        oerr = float((out.double() - ref["o"]).abs().max())
        obar = 2e-2 * float(ref["o"].abs().max()) + 1e-3
        rl2 = float((out.double() - ref["o"]).norm() / ref["o"].norm())
        lerr = float((lse.double() - ref["lse"]).abs().max())
        r_out, r_lse[kind] = A.ratio(out, ref["o"], fwd["o"]), A.ratio(lse, ref["lse"], fwd["lse"])
        print("[control] leak on %s S 1025: out max err %.2g (old bar %.2g), rel-L2 %.2g (old bar 6e-3), lse err %.2g (old bar 2e-3); wide bars: out %.3g, lse %.3g"
              % (kind, oerr, obar, rl2, lerr, r_out, r_lse[kind]))
        assert oerr < obar and rl2 < 6e-3 and lerr < 2e-3
    assert r_lse["zeroq"] > 1.0
