"""LightningDiT's attention beyond the 288 tokens the resident kernels hold in LDS (-m gpu): the streaming kernels of csrc/attention_stream.hip and
csrc/attention_bwd_stream.hip on the head-major operands `ops.qknorm_rope` produces, head dims 64 and 72 (staged as 64 / 96), rows padded to 32 channels or not
(reference: F.scaled_dot_product_attention in diffusion/lightningdit/lightningdit.py:76-88 and its autograd; a 24 x 24 latent grid at patch 1 is 576 tokens, 32 x 32
is 1024).

Bars.  Forward, against float64 softmax attention on the same bf16 operands: the resident heads kernel's (test_gpu_dit.py::test_fused_attention_heads_kernel: rel-L2
< 6e-3, max|err| < 2^-6 max|ref| + 1e-3) and |lse - logsumexp| < 2e-3 (test_gpu_attention_stream.py).  Backward, per component dq / dk / dv against float64
autograd: the D = 64 streaming backward's (test_gpu_attention_bwd_stream.py: rel-L2 < 1.2e-2, max-error / max < 3e-2, |.| < 1e-5 where the true gradient is
identically zero).  Module level: the bars of the tests named at each assertion.  Reruns and batch splits are bit-identical."""
import copy

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
RL2_FWD, LSE_BAR = 6e-3, 2e-3
RL2_BWD, REL_BWD, ZERO_BAR = 1.2e-2, 3e-2, 1e-5


def _rl2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _pad(t, d):
    """[BH, N, d] -> rows of d rounded up to 32 channels, zeros behind the real ones (what `ops.qknorm_rope(padded=True)` produces)"""
    dp = (d + 31) // 32 * 32
    return t if dp == d else torch.nn.functional.pad(t, (0, dp - d)).contiguous()


def _ref64(q, k, v, b, do=None):
    """q, k, v [B*H, N, D] bf16 -> float64 out [B, N, H*D], lse [B*H, N] of softmax(scale q k^T) v on the same values; with do [B, N, H*D] also (dq, dk, dv) by
    autograd."""
    bh, n, d = v.shape
    h = bh // b
    q64, k64, v64 = (t.double().clone().requires_grad_(do is not None) for t in (q, k, v))
    sc = q64 @ k64.transpose(1, 2) * d ** -0.5
    o = torch.softmax(sc, dim=-1) @ v64
    out = o.view(b, h, n, d).permute(0, 2, 1, 3).reshape(b, n, h * d)
    lse = torch.logsumexp(sc, dim=-1)
    if do is None:
        return out, lse
    out.backward(do.double())
    return out.detach(), lse.detach(), (q64.grad, k64.grad, v64.grad)


_CASES = {}


def _case(b, h, d, n, mult=1.5, zero_q=False):
    """(q, k, v, do, float64 out, lse, (dq, dk, dv)): computed once per shape and shared; nobody writes to them.  randn x mult in bf16."""
    key = (b, h, d, n, mult, zero_q)
    if key not in _CASES:
        g = torch.Generator().manual_seed(100000 * b + 1000 * n + 10 * h + d)
        q, k, v = (torch.randn(b * h, n, d, generator=g) * mult for _ in range(3))
        if zero_q:
            q = torch.zeros_like(q)
        q, k, v = (t.to(BF).to(DEV) for t in (q, k, v))
        do = torch.randn(b, n, h * d, generator=g).to(BF).to(DEV)
        _CASES[key] = (q, k, v, do) + _ref64(q, k, v, b, do)
    return _CASES[key]


def _check_fwd(fn, q, k, v, b, ref, lse_ref, tag):
    """fn(q, k, v, b, scale, need_lse=True) on unpadded rows against float64 at the resident kernel's bars; padded rows, a second call and the form without lse give
    the same bits.  Returns (out, lse)."""
    d = v.shape[-1]
    scale = d ** -0.5
    out, lse = fn(q, k, v, b, scale, need_lse=True)
    assert out.shape == ref.shape and out.dtype == BF and lse.shape == lse_ref.shape and lse.dtype == torch.float32
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), tag
    err, rl2, lerr = (out.double() - ref).abs().max().item(), _rl2(out, ref), (lse.double() - lse_ref).abs().max().item()
    bar = 2 ** -6 * ref.abs().max().item() + 1e-3
    print(f"{tag}: max|err| {err:.3e} (bar {bar:.3e})  rl2 {rl2:.3e}  lse err {lerr:.3e}")
    assert rl2 < RL2_FWD, (tag, rl2)
    assert err < bar, (tag, err)
    assert lerr < LSE_BAR, (tag, lerr)
    out_p, lse_p = fn(_pad(q, d), _pad(k, d), v, b, scale, need_lse=True)
    assert torch.equal(out_p, out) and torch.equal(lse_p, lse), tag + ": padded q / k rows"
    out2, lse2 = fn(q, k, v, b, scale, need_lse=True)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), tag + ": rerun"
    assert torch.equal(fn(q, k, v, b, scale), out), tag + ": the form without lse"
    return out, lse


# ---- 1. forward against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,d,n", [(1, 2, 72, 289),      # first length over the cap: one live query in the last query block, one live key in the last tile
                                     (1, 1, 72, 320),      # a multiple of 32 and 64: no masking
                                     (2, 2, 72, 576),      # a 24 x 24 latent grid
                                     (1, 2, 64, 577),      # the 64-wide instantiation on head-major operands, ragged
                                     (1, 2, 72, 1024)])    # a 32 x 32 latent grid
def test_heads_stream_forward_vs_float64_through_dispatch(b, h, d, n):
    from dmvae_amd import ops
    q, k, v, _, ref, lse_ref, _ = _case(b, h, d, n)
    assert ops.attention_heads_supported(n, d)
    _check_fwd(ops.attention_heads, q, k, v, b, ref, lse_ref, f"attention_heads {b}x{h}x{d}x{n}")


@pytest.mark.parametrize("b,h,d,n", [(2, 3, 72, 17),       # less than one tile
                                     (1, 2, 72, 1),        # a single key
                                     (1, 1, 64, 64)])      # exactly one tile
def test_heads_stream_forward_vs_float64_direct_short(b, h, d, n):
    from dmvae_amd import ops
    q, k, v, _, ref, lse_ref, _ = _case(b, h, d, n)
    _check_fwd(ops.attention_heads_stream, q, k, v, b, ref, lse_ref, f"attention_heads_stream {b}x{h}x{d}x{n}")


# ---- 2. inputs that force the rescale on every tile ------------------------------------------------------------------------------------
def _directed(n, h, d, kind, seed):
    """test_gpu_attention_stream.py::_directed on head-major operands: q, k, v [h, n, d] bf16 (batch 1).  Queries: g_i * u, g_i in [14, 16], one unit direction u
    per head.  Keys: coef_j * u -- 'ascending': coef rises linearly from 0 to 8 over j (scaled scores up to 16, every 64-key tile raises the running maximum);
    'last': the same coefficients x 0.2 except the last key = 8 u (scores <= 3.2, then 14 .. 16 on the very last key of the ragged last tile).  'zeroq': zero
    queries, random keys.  V: randn x 1.5."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(h, 1, d, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    gq = 14 + 2 * torch.rand(h, n, 1, generator=g)
    q = gq * u * (d / 64) ** 0.5          # the scale is d^-0.5: the same scaled scores as at head dim 64
    coef = torch.linspace(0, 8, n).view(1, n, 1)
    if kind == "last":
        coef = coef * 0.2
        coef[:, -1] = 8.0
    k = coef * u
    if kind == "zeroq":
        q = torch.zeros(h, n, d)
        k = torch.randn(h, n, d, generator=g) * 1.5
    v = torch.randn(h, n, d, generator=g) * 1.5
    return tuple(t.to(BF).to(DEV) for t in (q, k, v))


@pytest.mark.parametrize("n", [289, 576])
@pytest.mark.parametrize("kind", ["ascending", "last", "zeroq", "randn4"])
def test_heads_stream_forward_rescale_inputs(n, kind):
    from dmvae_amd import ops
    h, d = 2, 72
    if kind == "randn4":
        q, k, v = _case(1, h, d, n, mult=4.0)[:3]
    else:
        q, k, v = _directed(n, h, d, kind, n + len(kind))
    ref, lse_ref = _ref64(q, k, v, 1)
    bar = 2 ** -6 * ref.abs().max().item() + 1e-3
    v_rows = v.double().permute(1, 0, 2).reshape(1, n, h * d)          # [1, n, h*d]: V in the output's layout
    sc = q.double() @ k.double().transpose(1, 2) * d ** -0.5
    # the inputs do what they are meant to do (checked on the float64 reference)
    if kind == "ascending":      # the maximum of every 64-key tile exceeds the maximum of everything before it, for every query
        tiles = [sc[..., t:t + 64].max(dim=-1).values for t in range(0, n, 64)]
        assert all((tiles[i + 1] > tiles[i]).all() for i in range(len(tiles) - 1))
    if kind == "last":           # the last key takes (nearly) all the weight: every output row is V[n - 1]
        assert (sc[..., -1] - sc[..., :-1].max(dim=-1).values).min().item() > 9.0
        assert (ref - v_rows[:, -1:]).abs().max().item() < bar
    if kind == "zeroq":          # uniform weights: every output row is the mean of V
        assert sc.abs().max().item() == 0.0
    out, lse = _check_fwd(ops.attention_heads_stream, q, k, v, 1, ref, lse_ref, f"{kind} N={n}")
    if kind == "last":
        assert (out.double() - v_rows[:, -1:]).abs().max().item() < bar
    if kind == "zeroq":
        assert (out.double() - v_rows.mean(dim=1, keepdim=True)).abs().max().item() < bar


# ---- 3. backward against float64 autograd ---------------------------------------------------------------------------------------------
def _stream_bwd(q, k, v, do, b, padded=False):
    """forward (out, lse) from the streaming forward, then the streaming backward, both through their direct entries"""
    from dmvae_amd import ops
    d = v.shape[-1]
    if padded:
        q, k = _pad(q, d), _pad(k, d)
    out, lse = ops.attention_heads_stream(q, k, v, b, d ** -0.5, need_lse=True)
    return ops.attention_bwd_heads_stream(q, k, v, out, do, b, d ** -0.5, lse)


def _hold(got, want, tag, zero=()):
    """(dq, dk, dv) bf16 against the float64 gradients, per component; components named in `zero` have an identically zero true gradient"""
    for name, g, w in zip(("dq", "dk", "dv"), got, want):
        assert g.shape == w.shape and g.dtype == BF and torch.isfinite(g.float()).all(), (tag, name)
        if name in zero:
            assert w.abs().max().item() == 0.0, (tag, name)          # the input does what it is meant to
            print(f"{tag} {name}: max|.| {g.float().abs().max().item():.3e} (true gradient identically zero)")
            assert g.float().abs().max().item() < ZERO_BAR, (tag, name, g.float().abs().max().item())
            continue
        e, r = _rl2(g, w), rel_err(g, w)
        print(f"{tag} {name}: rl2 {e:.3e}  rel_err {r:.3e}")
        assert e < RL2_BWD, (tag, name, e)
        assert r < REL_BWD, (tag, name, r)


@pytest.mark.parametrize("b,h,d,n", [(1, 2, 72, 289), (1, 1, 72, 320), (2, 2, 72, 576), (1, 2, 64, 577),
                                     (2, 2, 72, 17), (1, 1, 72, 64)])      # the last two: below the cap, through the direct entry
def test_heads_stream_backward_vs_float64(b, h, d, n):
    q, k, v, do, _, _, want = _case(b, h, d, n)
    got = _stream_bwd(q, k, v, do, b)
    _hold(got, want, f"attention_bwd_heads_stream {b}x{h}x{d}x{n}")
    again = _stream_bwd(q, k, v, do, b)
    assert all(torch.equal(a, b_) for a, b_ in zip(got, again))          # fixed summation order
    # padded q / k rows: the same bits in the real columns, zeros in the padded columns of dq / dk
    dq_p, dk_p, dv_p = _stream_bwd(q, k, v, do, b, padded=True)
    dp = (d + 31) // 32 * 32
    assert dq_p.shape == (b * h, n, dp) and dk_p.shape == (b * h, n, dp)
    assert torch.equal(dq_p[..., :d], got[0]) and torch.equal(dk_p[..., :d], got[1]) and torch.equal(dv_p, got[2])
    if dp > d:
        assert float(dq_p[..., d:].float().abs().max()) == 0.0 and float(dk_p[..., d:].float().abs().max()) == 0.0


@pytest.mark.parametrize("n", [289, 576])
@pytest.mark.parametrize("kind", ["randn4", "zeroq"])
def test_heads_stream_backward_hard_inputs(n, kind):
    """randn x 4: near-one-hot probability rows (large, cancelling dP - delta); q = 0: uniform P, and dk = scale dS^T Q is identically zero."""
    b, h, d = 1, 2, 72
    q, k, v, do, _, _, want = _case(b, h, d, n, mult=4.0) if kind == "randn4" else _case(b, h, d, n, zero_q=True)
    _hold(_stream_bwd(q, k, v, do, b), want, f"{kind} N={n}", zero=("dk",) if kind == "zeroq" else ())


# ---- 4. the twin: the resident lse kernels where both apply ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [72, 64])
def test_heads_stream_agrees_with_the_resident_kernels_at_256_tokens(d):
    """Different tilings of one softmax: the streaming entries called directly and the resident lse kernels (what `ops.attention_heads` / `ops.attention_bwd_heads`
    reach at 256 tokens) on the same operands, at the bars of cases 1 and 3."""
    from dmvae_amd import ops
    b, h, n = 2, 2, 256
    q, k, v, do, _, _, _ = _case(b, h, d, n)
    scale = d ** -0.5
    res, res_lse = ops.attention_heads(q, k, v, b, scale, need_lse=True)
    st, st_lse = ops.attention_heads_stream(q, k, v, b, scale, need_lse=True)
    print(f"D={d} forward streaming vs resident: rl2 {_rl2(st, res):.3e}  lse {(st_lse - res_lse).abs().max().item():.3e}")
    assert _rl2(st, res) < RL2_FWD
    assert (st.double() - res.double()).abs().max().item() < 2 ** -6 * res.float().abs().max().item() + 1e-3
    assert (st_lse - res_lse).abs().max().item() < LSE_BAR
    res_g = ops.attention_bwd_heads(q, k, v, res, do, b, scale, lse=res_lse)
    st_g = ops.attention_bwd_heads_stream(q, k, v, res, do, b, scale, res_lse)
    for name, a, w in zip(("dq", "dk", "dv"), st_g, res_g):
        e, r = _rl2(a, w), rel_err(a, w)
        print(f"D={d} {name}: streaming vs resident rl2 {e:.3e}  rel_err {r:.3e}")
        assert e < RL2_BWD and r < REL_BWD, (name, e, r)


# ---- 5. determinism and batch independence --------------------------------------------------------------------------------------------
def test_heads_stream_batch_split_is_bit_identical():
    from dmvae_amd import ops
    b, h, d, n = 4, 2, 72, 325
    q, k, v, do, _, _, _ = _case(b, h, d, n)
    scale = d ** -0.5
    out, lse = ops.attention_heads_stream(q, k, v, b, scale, need_lse=True)
    full = ops.attention_bwd_heads_stream(q, k, v, out, do, b, scale, lse)
    assert all(torch.equal(a, b_) for a, b_ in zip(full, ops.attention_bwd_heads_stream(q, k, v, out, do, b, scale, lse)))
    outs, lses, grads = [], [], []
    for i in (0, 2):
        rows = slice(i * h, (i + 2) * h)
        qi, ki, vi = (t[rows].contiguous() for t in (q, k, v))
        oi, li = ops.attention_heads_stream(qi, ki, vi, 2, scale, need_lse=True)
        outs.append(oi); lses.append(li)
        grads.append(ops.attention_bwd_heads_stream(qi, ki, vi, oi, do[i:i + 2].contiguous(), 2, scale, li))
    assert torch.equal(out, torch.cat(outs)) and torch.equal(lse, torch.cat(lses))
    for j in range(3):
        assert torch.equal(full[j], torch.cat([grads[0][j], grads[1][j]]))


# ---- 6. dispatch -----------------------------------------------------------------------------------------------------------------------
def test_heads_dispatch_keeps_the_resident_kernels_up_to_288_tokens_and_streams_above():
    from dmvae_amd import ops, _lib
    b, h, d = 2, 2, 72
    scale = d ** -0.5
    L = _lib.lib()
    for n in (257, 288):
        q, k, v, do, _, _, _ = _case(b, h, d, n)
        # the resident C entries called through the C ABI, not through ops
        want = torch.empty(b, n, h * d, dtype=BF, device=DEV)
        want_lse = torch.empty(b * h, n, dtype=torch.float32, device=DEV)
        ops.check(L.dmvae_attention_heads_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), want.data_ptr(), want_lse.data_ptr(), b, n, h, d, d, float(scale),
                                                   ops._stream()), "attention_heads_bf16")
        got, got_lse = ops.attention_heads(q, k, v, b, scale, need_lse=True)
        assert torch.equal(got, want) and torch.equal(got_lse, want_lse), n
        want_nolse = torch.empty_like(want)
        ops.check(L.dmvae_attention_heads_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), want_nolse.data_ptr(), None, b, n, h, d, d, float(scale), ops._stream()),
                  "attention_heads_bf16")
        assert torch.equal(ops.attention_heads(q, k, v, b, scale), want_nolse), n
        for lse in (want_lse, None):      # both resident backward forms
            wq, wk, wv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            ops.check(L.dmvae_attention_bwd_heads_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), want.data_ptr(), do.data_ptr(), ops._ptr(lse), wq.data_ptr(),
                                                           wk.data_ptr(), wv.data_ptr(), b, n, h, d, d, float(scale), ops._stream()), "attention_bwd_heads_bf16")
            gq, gk, gv = ops.attention_bwd_heads(q, k, v, want, do, b, scale, lse=lse)
            assert torch.equal(gq, wq) and torch.equal(gk, wk) and torch.equal(gv, wv), (n, lse is None)
    q, k, v, do, _, _, _ = _case(1, 2, d, 289)
    a, a_lse = ops.attention_heads(q, k, v, 1, scale, need_lse=True)
    s, s_lse = ops.attention_heads_stream(q, k, v, 1, scale, need_lse=True)
    assert torch.equal(a, s) and torch.equal(a_lse, s_lse) and torch.equal(ops.attention_heads(q, k, v, 1, scale), s)
    ga = ops.attention_bwd_heads(q, k, v, a, do, 1, scale, lse=a_lse)
    gs = ops.attention_bwd_heads_stream(q, k, v, a, do, 1, scale, a_lse)
    assert all(torch.equal(x, y) for x, y in zip(ga, gs))
    with pytest.raises(ValueError):
        ops.attention_bwd_heads(q, k, v, a, do, 1, scale)                       # above the cap the row statistics are required
    with pytest.raises(ValueError):
        ops.attention_bwd_heads_stream(q, k, v, a, do, 1, scale, None)
    assert ops.attention_heads_supported(1024, 72) and ops.attention_heads_supported(1024, 64)
    assert not ops.attention_heads_supported(320, 40)
    assert ops.attention_heads_supported(288, 40) and ops.attention_heads_supported(96, 80)      # the other head dims keep their range


# ---- 7. module level, with the composed route made to raise ---------------------------------------------------------------------------
# hd72: the dit_small_hd72 fixture is width 144 = 2 heads x 72, and `dit_stack_supported` needs a width that is a multiple of 32; the width is DOUBLED here to
# 288 = 4 heads x 72 (same head dim, same block structure) so that the one-node stack route is taken.  hd64w: dit_small_hd64w's own width, 192 = 3 heads x 64.
_MODEL_CFGS = {"hd72": dict(hidden_size=288, num_heads=4), "hd64w": dict(hidden_size=192, num_heads=3)}


def _model(tag, seed=0):
    """LightningDiT, depth 2, a 24 x 24 grid at patch 1 = 576 tokens, EVERY parameter randomised -- the zero-initialised adaLN and final-layer weights included
    (with them at zero the output is identically zero)."""
    from dmvae_amd.models.lightningdit import LightningDiT
    torch.manual_seed(seed)
    m = LightningDiT(input_size=24, patch_size=1, in_channels=8, depth=2, num_classes=10, **_MODEL_CFGS[tag]).to(DEV).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name == "pos_embed":
                continue
            if "adaLN_modulation" in name:
                p.normal_(0, 0.02 if p.dim() > 1 else 0.3)
            elif "norm" in name:
                p.uniform_(0.7, 1.3)
            elif p.dim() > 1:
                p.normal_(0, p[0].numel() ** -0.5)
            else:
                p.normal_(0, 0.1)
    return m


def _inputs(b, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, 8, 24, 24, generator=g).to(DEV)
    return x, torch.rand(b, generator=g).to(DEV), torch.randint(0, 10, (b,), generator=g).to(DEV), torch.randn(b, 8, 24, 24, generator=g).to(DEV)


def _no_composed(monkeypatch):
    from dmvae_amd import ops

    def composed_route_is_gone(*args, **kwargs):
        raise AssertionError("the composed attention route (an N x N tensor in HBM) was taken")
    monkeypatch.setattr(ops, "softmax_rows", composed_route_is_gone)
    monkeypatch.setattr(ops, "softmax_rows_bwd", composed_route_is_gone)


@pytest.mark.parametrize("tag", ["hd72", "hd64w"])
def test_lightningdit_inference_at_576_tokens_streams(tag, monkeypatch):
    """(a) `model(x, t, y)` under no_grad and `forward_with_cfg` with the composed route made to raise; against `forward_stock` under autocast(bf16) at the bar of
    test_gpu_dit.py::test_lightningdit_xl1_fast_forward_shapes_and_determinism (rel-L2 < 3e-2); a 2B call equals two B calls bit for bit."""
    from dmvae_amd.models import lightningdit_fast as lf
    _no_composed(monkeypatch)
    m = _model(tag).requires_grad_(False)
    x, t, y, _ = _inputs(4)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        assert lf.supported(m, x) and m._takes_inference_route(x)
        out = m(x, t, y)
        halves = [m(x[i:i + 2], t[i:i + 2], y[i:i + 2]) for i in (0, 2)]
        stock = m.forward_stock(x, t, y)
        cfg = m.forward_with_cfg(x, t, y, 1.5)
        cfg_want = m.forward_with_cfg_composed(x, t, y, 1.5)
    assert out.shape == x.shape and out.dtype == BF and torch.isfinite(out.float()).all() and out.float().abs().max() > 0
    e = _rl2(out.float(), stock.float())
    print(f"{tag} 576 tokens: inference route vs stock autocast rel-L2 {e:.3e}")
    assert e < 3e-2, e
    assert torch.equal(out, torch.cat(halves))
    assert cfg.shape == x.shape and torch.isfinite(cfg.float()).all() and _rl2(cfg.float(), cfg_want.float()) < 3e-2


def _train_run(m, x, t, y, dy, stack=True, stock=False):
    from dmvae_amd.models import lightningdit_fast as lf
    m.zero_grad(set_to_none=True)
    xa = x.clone().requires_grad_(True)
    lf.STACK_FN = stack
    try:
        with torch.autocast("cuda", dtype=BF):
            out = m.forward_stock(xa, t, y) if stock else m(xa, t, y)
        (out.float() * dy).sum().backward()
    finally:
        lf.STACK_FN = True
    return out.detach(), xa.grad


_STOCK_RUNS = {}


@pytest.mark.parametrize("tag", ["hd72", "hd64w"])
def test_lightningdit_training_at_576_tokens_streams(tag, monkeypatch):
    """(b) with gradients and the composed route made to raise: `dit_stack_supported` holds and the stack route runs; output, dx and every parameter gradient
    against the stock modules under autocast(bf16) at the bars of test_gpu_dit.py::test_lightningdit_train_route_matches_stock_autocast (1e-2 / 3e-2 / 4e-2 rel-L2);
    the `DitBlockFn` route against the stack route at the bars of test_gpu_dit_stack.py::test_stack_route_equals_block_route (same output bits, dx 2e-3, parameter
    gradients 5e-3).  (c) the frozen-weights input-gradient route against (b)'s dx at the 2e-3 bar."""
    from dmvae_amd import functional as Fn
    m = _model(tag)
    ref, blk = copy.deepcopy(m), copy.deepcopy(m)
    x, t, y, dy = _inputs(2)
    outs, dxs = _train_run(ref, x, t, y, dy, stock=True)          # the reference first: the patches below do not touch it, but it need not know about them
    _no_composed(monkeypatch)
    assert Fn.dit_stack_supported(2, 576, m.hidden_size, m.num_heads)      # at width 288 = 4 x 72 and at 192 = 3 x 64
    calls = []
    real_supported = Fn.dit_stack_supported
    monkeypatch.setattr(Fn, "dit_stack_supported", lambda *a: (calls.append(real_supported(*a)), calls[-1])[1])      # what forward_train decides the route by
    out, dx = _train_run(m, x, t, y, dy)
    assert calls == [True], "the stack route was not taken"
    e_out, e_dx = _rl2(out.float(), outs.float()), _rl2(dx, dxs)
    pa, pb, pc = dict(m.named_parameters()), dict(ref.named_parameters()), dict(blk.named_parameters())
    worst = max((n_ for n_ in pa if n_ != "pos_embed"), key=lambda n_: _rl2(pa[n_].grad, pb[n_].grad))
    print(f"{tag} 576 tokens, stack route vs stock autocast: out {e_out:.3e}  dx {e_dx:.3e}  worst parameter gradient {worst} {_rl2(pa[worst].grad, pb[worst].grad):.3e}")
    assert out.float().abs().max() > 0 and e_out < 1e-2, e_out
    assert e_dx < 3e-2, e_dx
    for n_, p in pa.items():
        if n_ == "pos_embed":
            continue
        assert p.grad is not None and pb[n_].grad.abs().max() > 0, n_
        assert _rl2(p.grad, pb[n_].grad) < 4e-2, (n_, _rl2(p.grad, pb[n_].grad))
    # the per-block route
    calls.clear()
    out_b, dx_b = _train_run(blk, x, t, y, dy, stack=False)
    assert not calls
    assert torch.equal(out_b, out)
    assert _rl2(dx, dx_b) < 2e-3, _rl2(dx, dx_b)
    for n_, p in pa.items():
        if n_ != "pos_embed":
            assert _rl2(p.grad, pc[n_].grad) < 5e-3, (n_, _rl2(p.grad, pc[n_].grad))
    # (c) frozen weights, a gradient for the input alone
    m.requires_grad_(False)
    m.zero_grad(set_to_none=True)
    out_f, dx_f = _train_run(m, x, t, y, dy)
    assert torch.equal(out_f, out)
    print(f"{tag} 576 tokens: frozen-weights dx vs the training route's rel-L2 {_rl2(dx_f, dx):.3e}")
    assert _rl2(dx_f, dx) < 2e-3, _rl2(dx_f, dx)


# ---- 8. memory -------------------------------------------------------------------------------------------------------------------------
def _block_forward_peak(b, n, heads, d, seed=0):
    """Bytes one `DitBlockFn` forward raises the allocation peak above the level just before it (a first call fills the weight caches and workspaces)."""
    from dmvae_amd import functional as Fn
    c, hid = heads * d, 32
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(DEV)
    h = r(b, n, c).requires_grad_(True)
    mod = (r(b, 6 * c, std=0.3)).to(BF)
    params = [1 + r(c, std=0.1), r(3 * c, c, std=c ** -0.5), r(3 * c, std=0.1), 1 + r(d, std=0.1), 1 + r(d, std=0.1), r(c, c, std=c ** -0.5), r(c, std=0.1),
              1 + r(c, std=0.1), r(2 * hid, c, std=c ** -0.5), r(2 * hid, std=0.1), r(c, hid, std=hid ** -0.5), r(c, std=0.1)]
    ang = torch.rand(n, d, generator=g) * 6.28
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    run = lambda: Fn.DitBlockFn.apply(h, mod, *params, cos, sin, heads, 1e-6)
    out = run()
    del out
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert torch.isfinite(out).all()
    return peak


def test_dit_block_forward_at_1024_tokens_saves_no_probabilities(monkeypatch):
    """One `DitBlockFn` forward at B = 1, H = 2 (D = 64), N = 1024 raises the allocation peak by less than B H N N 2 bytes -- the saved bf16 P alone -- and with
    `attention_heads_supported` forced back to n <= 288 (the composed route) by more: the condition discriminates."""
    from dmvae_amd import ops
    b, heads, d, n = 1, 2, 64, 1024
    p_bytes = b * heads * n * n * 2
    fused = _block_forward_peak(b, n, heads, d)
    print(f"DitBlockFn forward {b}x{heads}x{d}x{n}: peak allocation {fused / 2 ** 20:.2f} MiB fused (the saved bf16 P alone: {p_bytes / 2 ** 20:.2f} MiB)")
    assert fused < p_bytes, (fused, p_bytes)
    monkeypatch.setattr(ops, "attention_heads_supported", lambda n_, d_: n_ <= 288 and d_ % 8 == 0 and (d_ + 31) // 32 * 32 in (64, 96))
    composed = _block_forward_peak(b, n, heads, d)
    print(f"DitBlockFn forward {b}x{heads}x{d}x{n}: peak allocation {composed / 2 ** 20:.2f} MiB composed")
    assert composed > p_bytes, (composed, p_bytes)
