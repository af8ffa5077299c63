"""csrc/attention_wide_bwd.hip (-m gpu): the streaming BACKWARD of the decoder AttnBlock's attention -- ONE head of 512 channels (reference: autograd of
models/flux_ae.py:37-49) -- and its way up through functional.AttnBlockFn (above 1024 tokens) and VAE (288 px).

Bars are the sibling backward kernels' (tests/test_gpu_attention_bwd_stream.py), per component dq / dk / dv against float64 autograd of softmax(scale q k^T) v on the
same bf16 operands: rel-L2 < 1.2e-2 and max-error / max < 3e-2.  tests/test_attention_wide_bwd_emulation.py emulates the kernels' rounding sites in float64 (bf16
operands, f32 scores, dP and p, delta = sum_k P dP in f32, P rounded to bf16 once, scale * dS as hi + lo, one rounding at the store): rel-L2 <= 2.5e-3 and max-error /
max <= 9.4e-3 on every input family used here, so the bars leave 3 x or more for the f32 summation order and the forward's lse.  At S = 1 the true dq and
dk are zero and what the kernel leaves is the f32 cancellation of two 512-term dot products (dP - delta): held below 2^-8 max|dv|, less than one bf16 step of an
ordinary entry.  Reruns and batch splits are bit-identical."""
import warnings

import pytest
import torch

from conftest import rel_err
from test_gpu_attention_wide import _attn_block, _count_calls, _directed, _oracle_34, _raiser, _randn_qkv, _rl2

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
C = 512
SCALE = C ** -0.5
RL2_BAR, REL_BAR = 1.2e-2, 3e-2
NAMES = ("dq", "dk", "dv")


def _ref64(q, k, v, do):
    """float64 autograd of softmax(scale q k^T) v on the same bf16 values -> (dq, dk, dv) [B, S, 512]"""
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(SCALE * q @ k.transpose(-1, -2), dim=-1) @ v
    o.backward(do.double())
    return q.grad, k.grad, v.grad


_CASES = {}


def _case(b, s, kind="randn", mult=1.5):
    """(q, k, v, do, float64 reference): computed once per case and shared; nobody writes to them.  dO is randn."""
    key = (b, s, kind, mult)
    if key not in _CASES:
        if kind == "randn":
            q, k, v = _randn_qkv(b, s, mult, 1000 * s + b)
        elif kind == "zeroq":
            q, k, v = _randn_qkv(b, s, mult, 1000 * s + b + 1)
            q = torch.zeros_like(q)
        else:
            q, k, v = _directed(s, kind, s + len(kind))
        do = torch.randn(b, s, C, generator=torch.Generator().manual_seed(7 * s + b)).to(BF).to(DEV)
        _CASES[key] = (q, k, v, do, _ref64(q, k, v, do))
    return _CASES[key]


def _stream_bwd(q, k, v, do):
    """forward (o, lse) from the streaming forward, then the streaming backward through its direct entry"""
    from dmvae_amd import ops
    o, lse = ops.attention_wide_stream(q, k, v, SCALE, need_lse=True)
    return ops.attention_wide_bwd_stream(q, k, v, o, do, lse, SCALE)


def _hold(got, want, tag):
    errs = {}
    for name, g, w in zip(NAMES, got, want):      # every figure is printed before the first assertion
        assert g.shape == w.shape and g.dtype == BF and torch.isfinite(g.float()).all(), (tag, name)
        errs[name] = (_rl2(g, w), rel_err(g, w))
        print(f"{tag} {name}: rl2 {errs[name][0]:.3e}  rel_err {errs[name][1]:.3e}")
    for name, (e_l2, e_max) in errs.items():
        assert e_l2 < RL2_BAR, (tag, name, e_l2)
        assert e_max < REL_BAR, (tag, name, e_max)
    return errs


# ---- 1. the kernels against float64 autograd, direct entry ---------------------------------------------------------------------------
@pytest.mark.parametrize("b,s", [(2, 17),        # less than one tile
                                 (1, 31), (1, 32), (1, 33),      # one below, at and one above the 32 rows a workgroup owns in BOTH passes (= the 32-row tile)
                                 (1, 64), (1, 65),      # exactly two tiles / row blocks, and one row into the third
                                 (2, 1025),      # first token count over a power of two: one live row in the last tile and in the last row block
                                 (1, 1156),      # 34 x 34: ragged last tile and last row block
                                 (1, 2304)])     # 48 x 48 (384 px): several row blocks per XCD, no masking
def test_wide_backward_vs_float64(b, s):
    q, k, v, do, want = _case(b, s)
    got = _stream_bwd(q, k, v, do)
    _hold(got, want, f"attention_wide_bwd_stream {b}x{s}")
    again = _stream_bwd(q, k, v, do)
    assert all(torch.equal(g, a) for g, a in zip(got, again))          # fixed summation order


def test_wide_backward_of_a_single_key():
    """S = 1: the softmax is constant, dq = dk = 0 in exact arithmetic; dv = dO."""
    q, k, v, do, want = _case(1, 1)
    assert want[0].abs().max().item() == 0.0 and want[1].abs().max().item() == 0.0          # the input does what it is meant to
    dq, dk, dv = _stream_bwd(q, k, v, do)
    bar = 2 ** -8 * dv.float().abs().max().item()
    print(f"S=1: max|dq| {dq.float().abs().max().item():.3e}  max|dk| {dk.float().abs().max().item():.3e}  (bar 2^-8 max|dv| = {bar:.3e})")
    assert dq.float().abs().max().item() < bar and dk.float().abs().max().item() < bar
    assert _rl2(dv, want[2]) < RL2_BAR and rel_err(dv, want[2]) < REL_BAR
    again = _stream_bwd(q, k, v, do)
    assert all(torch.equal(g, a) for g, a in zip((dq, dk, dv), again))


# ---- 2. harder inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1025, 1156])
@pytest.mark.parametrize("kind", ["randn4", "zeroq", "ascending", "last"])
def test_wide_backward_hard_inputs(s, kind):
    """randn x 4: near-one-hot probability rows (large, cancelling dP - delta); q = 0: uniform P, and dk = scale dS^T Q is exactly zero; the forward test's directed
    inputs 'ascending' and 'last': the weight sits in the ragged last tile.

    On the directed inputs every key is a multiple of ONE direction u, so dq_i = scale (sum_j dS_ij coef_j) u with sum_j dS_ij = 0 and coef_j nearly constant over the
    keys that carry weight ('last': one key carries all of it): dq and dk are a few per cent of the terms they are summed from.  The sibling kernels' rounding sites
    (delta from the saved bf16 O, scale * dS rounded to bf16 once) miss these bars there -- dq rel-L2 4.4e-2 ... 0.86 in tests/test_attention_wide_bwd_emulation.py,
    and a build of these kernels with those two sites measured the same -- which is why csrc/attention_wide_bwd.hip forms delta = sum_k P dP in f32 from its own p
    and dP and feeds scale * dS to the matrix cores as hi + lo."""
    q, k, v, do, want = _case(1, s, mult=4.0) if kind == "randn4" else _case(1, s, kind)
    got = _stream_bwd(q, k, v, do)
    if kind == "zeroq":
        assert want[1].abs().max().item() == 0.0
        assert torch.equal(got[1], torch.zeros_like(got[1]))
        for name, g, w in ((NAMES[0], got[0], want[0]), (NAMES[2], got[2], want[2])):
            print(f"zeroq S={s} {name}: rl2 {_rl2(g, w):.3e}  rel_err {rel_err(g, w):.3e}")
            assert _rl2(g, w) < RL2_BAR and rel_err(g, w) < REL_BAR, name
    else:
        _hold(got, want, f"{kind} S={s}")


# ---- 3. no further from float64 than the composed route --------------------------------------------------------------------------------
def _composed_bwd(q, k, v, do):
    """dq, dk, dv from the ops functional.AttnBlockFn.backward calls on its composed route"""
    from dmvae_amd import functional as Fn, ops
    s = q.shape[1]
    sp = (s + 31) // 32 * 32
    q, k, v, do = Fn._attn_pad(q, sp), Fn._attn_pad(k, sp), Fn._attn_pad(v, sp), Fn._attn_pad(do, sp)
    p = Fn._attn_probs(q, k, SCALE, s)
    dp = ops.gemm_nt(do, v, out_f32=True)
    ds = ops.softmax_rows_bwd(dp, p, SCALE)
    dv = ops.gemm_tn(p, do)
    dq = ops.gemm_nt(ds, ops.transpose_last2(k))
    dk = ops.gemm_tn(ds, q)
    return dq[:, :s], dk[:, :s], dv[:, :s]


@pytest.mark.parametrize("b,s", [(2, 1156), (1, 2304)])
def test_wide_backward_twin_of_the_composed_route(b, s):
    q, k, v, do, want = _case(b, s)
    got, comp = _stream_bwd(q, k, v, do), _composed_bwd(q, k, v, do)
    for name, g, c, w in zip(NAMES, got, comp, want):
        e_stream, e_comp = _rl2(g, w), _rl2(c, w)
        print(f"S={s} {name}: streaming {e_stream:.3e}  composed {e_comp:.3e}")
        assert e_stream < 1.5 * e_comp + 5e-3, (name, e_stream, e_comp)


# ---- 4. batch independence -----------------------------------------------------------------------------------------------------------
def test_wide_backward_batch_split_is_bit_identical():
    q, k, v = _randn_qkv(4, 1089, 1.5, 1089)
    do = torch.randn(4, 1089, C, generator=torch.Generator().manual_seed(33)).to(BF).to(DEV)
    whole = _stream_bwd(q, k, v, do)
    halves = [_stream_bwd(*(t[i:i + 2].contiguous() for t in (q, k, v, do))) for i in (0, 2)]
    for j, name in enumerate(NAMES):
        assert torch.equal(whole[j], torch.cat([h[j] for h in halves])), name


# ---- 5. dispatch ---------------------------------------------------------------------------------------------------------------------
def _run(mod, x, dy, fwd=None, bwd=None):
    """forward + backward of the block with functional.ATTN_WIDE_STREAM = fwd and ATTN_WIDE_BWD_STREAM = bwd -> (y, dx, {name: grad})"""
    from dmvae_amd import functional as Fn
    mod.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    old = Fn.ATTN_WIDE_STREAM, Fn.ATTN_WIDE_BWD_STREAM
    Fn.ATTN_WIDE_STREAM, Fn.ATTN_WIDE_BWD_STREAM = fwd, bwd
    try:
        y = mod(x)
        y.backward(dy)
    finally:
        Fn.ATTN_WIDE_STREAM, Fn.ATTN_WIDE_BWD_STREAM = old
    return y.detach(), x.grad, {n: p.grad.clone() for n, p in mod.named_parameters()}


def _xdy(b, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, C, hw, hw, generator=g).to(DEV), torch.randn(b, C, hw, hw, generator=g).to(DEV)


def test_attnblock_default_route_streams_both_ways_and_never_composes(monkeypatch):
    from dmvae_amd import functional as Fn, ops
    mod = _attn_block(2)
    x, dy = _xdy(1, 34, 34)
    fwd, bwd = _count_calls(monkeypatch, "attention_wide_stream"), _count_calls(monkeypatch, "attention_wide_bwd_stream")
    monkeypatch.setattr(ops, "softmax_rows", _raiser("softmax_rows"))
    monkeypatch.setattr(ops, "softmax_rows_bwd", _raiser("softmax_rows_bwd"))
    monkeypatch.setattr(Fn, "_attn_probs", _raiser("_attn_probs"))
    _, dx, gs = _run(mod, x, dy)
    assert len(fwd) == 1 and len(bwd) == 1
    assert torch.isfinite(dx).all() and all(torch.isfinite(g).all() for g in gs.values())


def test_attnblock_backward_switch(monkeypatch):
    """The forward forced alone keeps the composed backward (the combination tests/test_gpu_attention_wide.py pins bit for bit); forced together with the backward switch
    it streams; False never streams; 32 x 32 tokens and the parity mode never reach the new op."""
    from dmvae_amd import parity
    mod = _attn_block(2)
    x, dy = _xdy(1, 34, 34)
    bwd = _count_calls(monkeypatch, "attention_wide_bwd_stream")
    pinned = _run(mod, x, dy, fwd=True, bwd=None)
    assert len(bwd) == 0
    forced = _run(mod, x, dy, fwd=True, bwd=True)
    assert len(bwd) == 1
    assert torch.equal(forced[0], pinned[0]) and _rl2(forced[1], pinned[1]) < 3e-2          # the same forward bits; dx by another backward
    off = _run(mod, x, dy, fwd=None, bwd=False)
    assert len(bwd) == 1
    assert torch.equal(off[0], pinned[0]) and torch.equal(off[1], pinned[1])                # streaming forward + composed backward, as pinned
    _run(mod, x, dy, fwd=False, bwd=True)                                                  # a composed forward saved P and has no lse
    assert len(bwd) == 1
    x32, dy32 = _xdy(1, 32, 32)
    _run(mod, x32, dy32)
    assert len(bwd) == 1
    with parity.enabled(True):
        _, dxp, _ = _run(mod, x, dy)
    assert len(bwd) == 1 and torch.isfinite(dxp).all()


# ---- 6. AttnBlock on the default route against the float64 oracle ---------------------------------------------------------------------------
def test_attnblock_default_route_at_34x34_against_the_float64_oracle():
    """tests/test_gpu_attention_wide.py's oracle case (its module, its inputs, its bars relative to the tensor's max-abs: 8e-3 against the oracle with bf16 rounding at
    the storage sites, 3e-2 against the oracle without; the analytically zero k.bias.grad held to the same fraction of its twin q.bias.grad), with both switches None:
    streaming forward AND streaming backward.  A rerun is bit-identical in y, dx and every gradient."""
    mod = _attn_block(5, qk_gain=0.7)
    x, dy = _xdy(1, 34, 1156)
    y, dx, gs = _run(mod, x, dy)
    exact = _oracle_34(mod, x, dy, False)[2]
    for sites, tol in ((True, 8e-3), (False, 3e-2)):
        yo, dxo, go = _oracle_34(mod, x, dy, sites)
        errs = {"y": rel_err(y.cpu(), yo), "dx": rel_err(dx.cpu(), dxo)}
        for n in go:
            if exact[n].abs().max() < 1e-4:    # analytically zero in float64 (the key bias shifts every score of a row alike)
                twin = exact[n.replace("k.", "q.", 1)].abs().max().item()
                print(f"{n}: max |grad| {gs[n].abs().max().item():.2e} (exactly zero in float64; bar {tol:g} x max|{n.replace('k.', 'q.', 1)}.grad| = {tol * twin:.2e})")
                assert n.startswith("k.") and gs[n].abs().max().item() < tol * twin, n
                continue
            errs[n] = rel_err(gs[n].cpu(), go[n])
        print(f"AttnBlock(512) 34x34 streaming both ways vs oracle {'with bf16 sites' if sites else 'float64'}: " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        for n, e in errs.items():
            assert e < tol, (n, e, tol)
    y2, dx2, gs2 = _run(mod, x, dy)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and all(torch.equal(gs[n], gs2[n]) for n in gs)


# ---- 7. memory -----------------------------------------------------------------------------------------------------------------------
def test_attnblock_backward_at_4096_tokens_peaks_a_score_tensor_per_sample_lower():
    """AttnBlock(512) at 64 x 64 tokens, b = 2: the peak above the starting point over forward + backward on the default route against the same with the composed
    backward (an f32 and a bf16 [b, S, S] score tensor, an f32 dP and a bf16 dS: 12 S^2 bytes per sample).  Asked: at least one f32 score tensor per sample less."""
    from dmvae_amd import functional as Fn
    mod = _attn_block(4)
    s, b = 4096, 2
    g = torch.Generator().manual_seed(64)
    warm = torch.randn(1, 34, 34, C, generator=g).to(BF).to(DEV)
    x = torch.randn(b, 64, 64, C, generator=g).to(BF).to(DEV)
    dy = torch.randn(b, 64, 64, C, generator=g).to(BF).to(DEV)

    def peak(bwd):
        old = Fn.ATTN_WIDE_BWD_STREAM
        Fn.ATTN_WIDE_BWD_STREAM = bwd
        try:
            mod.forward_nhwc(warm.clone().requires_grad_(True)).backward(torch.ones_like(warm))      # packed weights and workspaces exist before the measurement
            mod.zero_grad(set_to_none=True)
            xin = x.clone().requires_grad_(True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            mod.forward_nhwc(xin).backward(dy)
            torch.cuda.synchronize()
            assert torch.isfinite(xin.grad.float()).all()
            return torch.cuda.max_memory_allocated() - before
        finally:
            Fn.ATTN_WIDE_BWD_STREAM = old

    p_stream, p_comp = peak(None), peak(False)
    print(f"AttnBlock(512) {b}x64x64 forward + backward: peak {p_stream / 2**20:.1f} MiB streaming, {p_comp / 2**20:.1f} MiB with the composed backward "
          f"(asked: {b * s * s * 4 / 2**20:.1f} MiB less)")
    assert p_stream <= p_comp - b * s * s * 4


# ---- 8. VAE at 288 px ----------------------------------------------------------------------------------------------------------------
def test_vae_step_at_288_px_takes_the_streaming_backward_once(monkeypatch):
    from dmvae_amd.models.vae import VAE
    torch.manual_seed(288)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = VAE(z_channels=32, model_size="base", encoder_kwargs=dict(embed_dim=256, depth=1, num_heads=4, img_size=288)).to(DEV)
    x = torch.randn(1, 3, 288, 288, generator=torch.Generator().manual_seed(1)).clamp_(-1, 1).to(DEV)
    calls = _count_calls(monkeypatch, "attention_wide_bwd_stream")

    def step():
        vae.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF):
            y = vae(x)
        y.square().mean().backward()
        for n, p in vae.named_parameters():
            assert not p.requires_grad or (p.grad is not None and torch.isfinite(p.grad).all()), n
        return y.detach(), {n: p.grad.clone() for n, p in vae.named_parameters() if p.requires_grad}

    y1, g1 = step()
    assert len(calls) == 1
    y2, g2 = step()
    assert len(calls) == 2
    assert torch.equal(y1, y2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
