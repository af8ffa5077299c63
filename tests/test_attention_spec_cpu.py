"""tests/attention_spec.py without a GPU: the fp64 definitions against torch autograd, every input class against its purpose, the f32 / bf16 emulations of the
resident attention kernels (in kernel order) inside every bar on every shared case, and the negative controls -- one-line mutants of the emulations that have to
leave a bar.  The emulations are the only arbiter of the bars' width; nothing here leaves an element out.

Worst |error| / bound of the emulations over every shared case (tokens 1 .. 288 x head dims 40, 64, 72, 96 x the input classes; printed by
test_emulations_stay_inside_every_bar): out 0.744, lse 0.065, dq 0.334, dk 0.388, dv 0.876, the same for the forms with and without lse; the NR entry's out 0.482
(d = 64) and 0.574 (d = 72), with 0.2 % of the staged q / k values next to a tie.  No bar needed widening.
Negative controls (test_negative_controls prints every ratio): worst |error| / bound of each one-line mutant, on the case that tells it best --
  leak (one padded key unmasked)             out 122, lse 1.7e5 on `negative` S 33; on randn S 257 out stays at 0.54 and lse alone tells it (22)
  mask_last (the last live key masked)       out 3.1e3, lse 1.5e5 on `last` S 33
  lse_noscale (lse without scale on the max) lse 1.2e6
  half_max (row maximum over one half-wave)  infinite on `spike` (the power overflows); on randn4 it is the same softmax and stays inside (0.86)
  sum_rounded (sum of the bf16-rounded e)    lse 37; out stays inside (0.69)
  delta_other_head                           dq 123, dk 42
  dk_noscale                                 dk 270
  ds_round_first (d = 72)                    NOT told: dq 0.20, dk 0.36 (see UNTOLD)"""
import pytest
import torch

import attention_spec as A
from attention_spec import BF

B, H = 2, 3
DIMS = [40, 64, 72, 96]


def _shared_cases():
    return [(kind, s, d) for d in DIMS for s in A.TOKENS for kind in A.classes_at(s)]


def _all(c):
    ref = A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"])
    fwd = A.bars_forward(c["q"], c["k"], c["v"], c["scale"], ref)
    bwd = A.bars_backward(c["q"], c["k"], c["v"], c["do"], c["scale"], ref, fwd)
    return ref, fwd, bwd


# ---- the definitions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,s,d", [("randn", 33, 64), ("randn4", 65, 72), ("randn", 257, 64), ("negative", 31, 40), ("offset", 33, 96), ("zeroq", 33, 72)])
def test_spec_gradients_match_float64_autograd(kind, s, d):
    """(not on `last` / `spike`: with one probability at 1 - 1e-5 and less, dq and dk are differences of terms 1e4 times their size, and two correct fp64
    evaluations agree to 1e-16 of the TERMS, which is 2e-12 of the result)"""
    c = A.make_case(kind, B, H, s, d)
    ref = A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"])
    q, k, v = (c[n].double().requires_grad_(True) for n in "qkv")
    o = torch.softmax(c["scale"] * q @ k.transpose(-1, -2), -1) @ v
    o.backward(c["do"].double())
    for name, got, want in (("o", ref["o"], o.detach()), ("dq", ref["dq"], q.grad), ("dk", ref["dk"], k.grad), ("dv", ref["dv"], v.grad)):
        rel = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
        assert rel <= 1e-12, (name, rel)


def test_layout_helpers_round_trip():
    c = A.make_case("randn", B, H, 33, 64)
    q, k, v = A.from_packed(A.to_packed(c["q"], c["k"], c["v"], B, H), B, H)
    assert torch.equal(q, c["q"]) and torch.equal(k, c["k"]) and torch.equal(v, c["v"])
    assert torch.equal(A.from_rows(A.to_rows(c["do"], B, H), B, H), c["do"])
    p = A.pad_rows(c["q"], 96)
    assert p.shape[-1] == 96 and torch.equal(p[..., :64], c["q"]) and float(p[..., 64:].abs().max()) == 0
    qkv = A.to_packed(c["q"], c["k"], c["v"], B, H).view(B, 33, 3, H, 64)      # item g = b * H + h
    assert torch.equal(qkv[1, :, 1, 2], c["k"][1 * H + 2])


def test_every_class_does_what_it_is_for():
    for kind, s, d in _shared_cases():
        c = A.make_case(kind, B, H, s, d)
        A.check_class(c, A.reference(c["q"], c["k"], c["v"], c["do"], c["scale"]))


def test_spread_items_cover_every_remap_class():
    for total in (512, 520, 552, 648):
        it = A.spread_items(total)
        assert len(it) >= 24 and it[0] == 0 and it[-1] == total - 1 and len(set(it)) == len(it)
        inv = {A.xcd_remap(f, total): f for f in range(total)}
        assert sorted(inv) == list(range(total))                                 # the remap is a permutation
        assert {inv[i] & 7 for i in it} == set(range(8))


# ---- the emulations inside the bars ---------------------------------------------------------------------------------------------------------------
def _hold_case(c, tag):
    ref, fwd, bwd = _all(c)
    out, lse = A.emulate_forward(c["q"], c["k"], c["v"], c["scale"])
    A.hold(out, ref["o"], fwd["o"], tag + " out", "out")
    A.hold(lse, ref["lse"], fwd["lse"], tag + " lse", "lse")
    for form, l in (("lse", lse), ("no lse", None)):
        dq, dk, dv = A.emulate_backward(c["q"], c["k"], c["v"], out, c["do"], c["scale"], lse=l)
        for n, g in (("dq", dq), ("dk", dk), ("dv", dv)):
            A.hold(g, ref[n], bwd[n], "%s %s (%s)" % (tag, n, form), "%s (%s)" % (n, form))


def test_emulations_stay_inside_every_bar():
    A.FIG.clear()
    for kind, s, d in _shared_cases():
        _hold_case(A.make_case(kind, B, H, s, d), "%s S %d d %d" % (kind, s, d))
    for k, v in A.FIG.items():
        print("[fig] %s: worst emulation |err| / bound %.3f (bar 1)" % (k, v))
    assert A.FIG and max(A.FIG.values()) <= 1.0


@pytest.mark.parametrize("d", [64, 72])
def test_nr_emulation_stays_inside_its_bar(d):
    A.FIG.clear()
    for s in (1, 33, 256, 288):
        c = A.make_case("randn", B, H, s, d, seed=5)
        qkv = A.to_packed(c["q"], c["k"], c["v"], B, H)
        qw, kw, cos, sin = A.nr_tables(s, d, 0)
        q, k, v, dq_, dk_ = A.nr_operands(qkv, qw, kw, cos, sin, H, 1e-6)
        ref = A.reference(q, k, v, c["do"], c["scale"])
        fwd = A.bars_forward(q, k, v, c["scale"], ref, dqk=(dq_, dk_))
        qe, ke, ve = A.emulate_nr_operands(qkv, qw, kw, cos, sin, H, 1e-6)
        assert torch.equal(ve, v)
        assert bool(((qe.double() - q.double()).abs() <= dq_).all()) and bool(((ke.double() - k.double()).abs() <= dk_).all()), "staged q / k outside the tie slack"
        out, _ = A.emulate_forward(qe, ke, ve, c["scale"])
        A.hold(out, ref["o"], fwd["o"], "NR S %d d %d" % (s, d), "NR out")
        frac = float(((dq_ > 0).double().mean() + (dk_ > 0).double().mean()) / 2)
        print("[fig] NR S %d d %d: share of staged q / k values next to a tie %.4f" % (s, d, frac))
    print("[fig] NR out: worst emulation |err| / bound %.3f (bar 1)" % A.FIG["NR out"])


# ---- negative controls ----------------------------------------------------------------------------------------------------------------------
# name -> (which emulation, the cases it is run on).  Each is one changed line of the emulation (attention_spec.emulate_*: `mutant`).
CONTROLS = {
    "leak": ("fwd", [("negative", 33, 64), ("negative", 257, 64), ("randn", 257, 64), ("negative", 200, 72)]),
    "mask_last": ("fwd", [("last", 33, 64), ("last", 257, 64), ("randn", 257, 64)]),
    "lse_noscale": ("fwd", [("randn", 33, 64), ("offset", 257, 72)]),
    "half_max": ("fwd", [("spike", 33, 64), ("spike", 257, 64), ("spike", 288, 72), ("randn4", 257, 64)]),
    "sum_rounded": ("fwd", [("randn", 33, 64), ("randn4", 257, 64), ("zeroq", 257, 72), ("randn", 31, 40)]),
    "delta_other_head": ("bwd", [("randn", 33, 64), ("last", 257, 72)]),
    "dk_noscale": ("bwd", [("randn", 33, 64), ("negative", 257, 72)]),
    "ds_round_first": ("bwd", [("randn", 33, 72), ("randn4", 257, 72), ("randn", 31, 72), ("randn", 1, 72)]),
}
# Controls the bars cannot tell from the kernel's order, with the reason; test_negative_controls prints the measured worst ratio next to each.
#   ds_round_first  a second bf16 rounding of dS doubles one site's half-ulp per element, but the bar takes that site's errors at their worst-case sum over the keys
#                   while they add up like a random walk: dq 0.20, dk 0.36 of the bar at worst, where the kernel's order gives 0.33 and 0.39 over all cases.
# (sum_rounded leaves `out` inside its bar, 0.69 at worst -- numerator and denominator stay consistent -- and is told by lse, whose sum it is: 4 to 37 times the bar.)
UNTOLD = {"ds_round_first"}


def _control_ratio(name, kind, s, d):
    form, _ = CONTROLS[name]
    c = A.make_case(kind, B, H, s, d)
    ref, fwd, bwd = _all(c)
    if form == "fwd":
        out, lse = A.emulate_forward(c["q"], c["k"], c["v"], c["scale"], mutant=name)
        return {"out": A.ratio(out, ref["o"], fwd["o"]), "lse": A.ratio(lse, ref["lse"], fwd["lse"])}
    out, lse = A.emulate_forward(c["q"], c["k"], c["v"], c["scale"])
    dq, dk, dv = A.emulate_backward(c["q"], c["k"], c["v"], out, c["do"], c["scale"], lse=lse, mutant=name)
    return {n: A.ratio(g, ref[n], bwd[n]) for n, g in (("dq", dq), ("dk", dk), ("dv", dv))}


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_negative_controls(name):
    worst = 0.0
    for kind, s, d in CONTROLS[name][1]:
        r = _control_ratio(name, kind, s, d)
        worst = max(worst, max(r.values()))
        print("[control] %s on %s S %d d %d: %s" % (name, kind, s, d, ", ".join("%s %.3g" % kv for kv in r.items())))
    if name in UNTOLD:
        print("[control] %s: NOT told from the kernel's order by the bars, worst ratio %.3g (see UNTOLD)" % (name, worst))
        assert worst <= 1.0, "the bars do tell %s: take it out of UNTOLD" % name
    else:
        assert worst > 1.0, "%s stays inside every bar (worst ratio %.3g)" % (name, worst)


def test_leaked_key_is_caught_where_the_whole_tensor_bars_were_blind():
    """randn x 1.5 at S = 257 (the ViT shape): rel-L2 < 6e-3 and |lse err| < 2e-3 pass with a padded key unmasked; the lse bar does not"""
    c = A.make_case("randn", B, H, 257, 64)
    ref, fwd, _ = _all(c)
    out, lse = A.emulate_forward(c["q"], c["k"], c["v"], c["scale"], mutant="leak")
    rl2 = float((out.double() - ref["o"]).norm() / ref["o"].norm())
    lerr = float((lse.double() - ref["lse"]).abs().max())
    print("[control] leak on randn S 257: rel-L2 %.3g (old bar 6e-3), lse err %.3g (old bar 2e-3), lse ratio %.3g" % (rl2, lerr, A.ratio(lse, ref["lse"], fwd["lse"])))
    assert rl2 < 6e-3 and lerr < 2e-3
    assert A.ratio(lse, ref["lse"], fwd["lse"]) > 1.0
