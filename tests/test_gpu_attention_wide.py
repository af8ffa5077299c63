"""csrc/attention_wide.hip (-m gpu): the decoder AttnBlock's attention -- ONE head of 512 channels (reference models/flux_ae.py:37-49) -- streamed in 32-key
K / V tiles with an online softmax, and its way up through functional.AttnBlockFn (above 1024 tokens), Decoder (any square token grid) and VAE (288 px).

Bars are the ones the other attention kernels are held to (tests/test_gpu_attention_stream.py): max|err| < 2e-2 max|ref| + 1e-3, rel-L2 < 6e-3 and
|lse - logsumexp| < 2e-3, all against float64 softmax attention on the same bf16 operands; reruns and batch splits bit-identical.  The directed inputs make every
tile raise the running maximum, so the rescale of the accumulators is exercised on every step."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
C = 512
SCALE = C ** -0.5


def _rl2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _ref64(q, k, v):
    """q, k, v [B, S, 512] bf16 -> float64 (out [B, S, 512], lse [B, S]) of softmax(scale q k^T) v on the same values."""
    sc = q.double() @ k.double().transpose(-2, -1) * SCALE
    return torch.softmax(sc, dim=-1) @ v.double(), torch.logsumexp(sc, dim=-1)


def _bar(ref):
    return 2e-2 * ref.abs().max().item() + 1e-3


def _check(q, k, v, tag):
    """ops.attention_wide_stream against float64 at the project's bars; a second call bit-identical; the form without lse the same out.  Returns (out, ref)."""
    from dmvae_amd import ops
    out, lse = ops.attention_wide_stream(q, k, v, SCALE, need_lse=True)
    ref, lse_ref = _ref64(q, k, v)
    assert out.shape == ref.shape and out.dtype == BF and lse.shape == lse_ref.shape and lse.dtype == torch.float32
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), tag
    err, rl2, lerr = (out.double() - ref).abs().max().item(), _rl2(out, ref), (lse.double() - lse_ref).abs().max().item()
    print(f"{tag}: max|err| {err:.3e} (bar {_bar(ref):.3e})  rl2 {rl2:.3e}  lse err {lerr:.3e}")
    assert err < _bar(ref), (tag, err)
    assert rl2 < 6e-3, (tag, rl2)
    assert lerr < 2e-3, (tag, lerr)
    out2, lse2 = ops.attention_wide_stream(q, k, v, SCALE, need_lse=True)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), tag
    assert torch.equal(ops.attention_wide_stream(q, k, v, SCALE), out), tag + ": the form without lse"
    return out, ref


def _randn_qkv(b, s, mult, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(b, s, C, generator=g) * mult).to(BF).to(DEV) for _ in range(3))


# ---- 1. the kernel against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,s", [(1, 1),         # a single key
                                 (2, 17),        # less than one tile
                                 (1, 32), (1, 33),      # exactly one 32-key tile, and one key into the second
                                 (1, 64), (1, 65),      # exactly one 64-query block, and one query into the second
                                 (2, 1025),      # first token count over a power of two: one live key in the last tile, one live query in the last block
                                 (1, 1156),      # 34 x 34: ragged last tile and last query block
                                 (1, 2304)])     # 48 x 48 (384 px): several query blocks per XCD, no masking
def test_wide_attention_vs_float64(b, s):
    _check(*_randn_qkv(b, s, 1.5, 1000 * s + b), f"attention_wide_stream {b}x{s}")


# ---- 2. inputs that force the rescale on every tile ------------------------------------------------------------------------------------
def _directed(s, kind, seed):
    """tests/test_gpu_attention_stream.py's _directed for one head of 512 channels, q and k each multiplied by 8^(1/4) so that the scaled scores reach 16 as they
    do at d = 64.  Queries: g_i * u, g_i in [14, 16], u a unit direction.  Keys: coef_j * u -- 'ascending': coef rises linearly from 0 to 8 over j (every 32-key tile
    raises the running maximum); 'last': the same coefficients x 0.2 except the last key = 8 u (the very last key of the ragged last tile takes the weight).
    'zeroq': zero queries, random keys.  V: randn x 1.5."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(C, generator=g)
    u = u / u.norm()
    amp = 8 ** 0.25
    q = (14 + 2 * torch.rand(s, 1, generator=g)) * u * amp
    coef = torch.linspace(0, 8, s).view(s, 1)
    if kind == "last":
        coef = coef * 0.2
        coef[-1] = 8.0
    k = coef * u * amp
    if kind == "zeroq":
        q = torch.zeros(s, C)
        k = torch.randn(s, C, generator=g) * 1.5
    v = torch.randn(s, C, generator=g) * 1.5
    return tuple(t.reshape(1, s, C).to(BF).to(DEV) for t in (q, k, v))


@pytest.mark.parametrize("s", [1025, 1156])
@pytest.mark.parametrize("kind", ["ascending", "last", "zeroq", "randn4"])
def test_wide_attention_rescale_inputs(s, kind):
    q, k, v = _randn_qkv(1, s, 4.0, s + 7) if kind == "randn4" else _directed(s, kind, s + len(kind))
    out, ref = _check(q, k, v, f"{kind} S={s}")
    vd = v.double()
    if kind == "last":          # the last key takes (nearly) all the weight: every output row is V[S - 1]
        assert (ref - vd[:, -1:]).abs().max().item() < _bar(ref)       # the inputs do what they are meant to
        assert (out.double() - vd[:, -1:]).abs().max().item() < _bar(ref)
    if kind == "zeroq":         # uniform weights: every output row is the mean of V
        assert (out.double() - vd.mean(dim=1, keepdim=True)).abs().max().item() < _bar(ref)


# ---- 3. batch independence -----------------------------------------------------------------------------------------------------------
def test_wide_attention_batch_split_is_bit_identical():
    from dmvae_amd import ops
    q, k, v = _randn_qkv(4, 1089, 1.5, 1089)
    out, lse = ops.attention_wide_stream(q, k, v, SCALE, need_lse=True)
    halves = [ops.attention_wide_stream(q[i:i + 2].contiguous(), k[i:i + 2].contiguous(), v[i:i + 2].contiguous(), SCALE, need_lse=True) for i in (0, 2)]
    assert torch.equal(out, torch.cat([h[0] for h in halves])) and torch.equal(lse, torch.cat([h[1] for h in halves]))


# ---- 4 / 5. AttnBlock: dispatch, and the two routes against each other ---------------------------------------------------------------------
def _attn_block(seed, qk_gain=1.5):
    """AttnBlock(512) with randomised norm and conv weights (the default initialisation has unit norm weights and zero biases).  qk_gain: the q / k convs' weight
    scale -- 1.5 gives scaled scores of standard deviation ~2, a smaller one a flatter softmax."""
    from dmvae_amd.models.flux_ae import AttnBlock
    torch.manual_seed(seed)
    mod = AttnBlock(C)
    with torch.no_grad():
        mod.norm.weight.uniform_(0.5, 1.5)
        mod.norm.bias.normal_(0, 0.2)
        for conv in (mod.q, mod.k, mod.v, mod.proj_out):
            conv.weight.normal_(0, (qk_gain if conv in (mod.q, mod.k) else 1.5) * C ** -0.5)
            conv.bias.normal_(0, 0.2)
    return mod.to(DEV)


def _run(mod, x, dy, route):
    """forward + backward of the block with functional.ATTN_WIDE_STREAM = route -> (y, dx, {name: grad})"""
    from dmvae_amd import functional as Fn
    mod.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    old = Fn.ATTN_WIDE_STREAM
    Fn.ATTN_WIDE_STREAM = route
    try:
        y = mod(x)
        y.backward(dy)
    finally:
        Fn.ATTN_WIDE_STREAM = old
    return y.detach(), x.grad, {n: p.grad.clone() for n, p in mod.named_parameters()}


def _count_calls(monkeypatch, name):
    from dmvae_amd import ops
    calls, real = [], getattr(ops, name)

    def counted(*a, **kw):
        calls.append(name)
        return real(*a, **kw)
    monkeypatch.setattr(ops, name, counted)
    return calls


def _raiser(name):
    def fn(*a, **kw):
        raise AssertionError(f"ops.{name} must not be called on this route")
    return fn


def test_attnblock_keeps_the_composed_route_up_to_1024_tokens(monkeypatch):
    from dmvae_amd import ops
    mod = _attn_block(1)
    g = torch.Generator().manual_seed(32)
    x, dy = torch.randn(1, C, 32, 32, generator=g).to(DEV), torch.randn(1, C, 32, 32, generator=g).to(DEV)
    want = _run(mod, x, dy, False)
    monkeypatch.setattr(ops, "attention_wide_stream", _raiser("attention_wide_stream"))
    got = _run(mod, x, dy, None)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for n in want[2]:
        assert torch.equal(got[2][n], want[2][n]), n


def test_attnblock_streams_above_1024_tokens_and_not_in_parity_mode(monkeypatch):
    from dmvae_amd import ops, parity
    mod = _attn_block(2)
    g = torch.Generator().manual_seed(34)
    x, dy = torch.randn(1, C, 34, 34, generator=g).to(DEV), torch.randn(1, C, 34, 34, generator=g).to(DEV)
    calls = _count_calls(monkeypatch, "attention_wide_stream")
    _run(mod, x, dy, None)
    assert len(calls) == 1
    with monkeypatch.context() as m, torch.no_grad():       # nothing S x S in a forward without a graph: the composed softmax is never reached
        m.setattr(ops, "softmax_rows", _raiser("softmax_rows"))
        mod(x)
    assert len(calls) == 2
    with parity.enabled(True), torch.no_grad():
        y = mod(x)
    assert len(calls) == 2 and y.dtype == torch.float32 and torch.isfinite(y).all()


def test_attnblock_streaming_route_against_the_composed_route():
    mod = _attn_block(3)
    g = torch.Generator().manual_seed(3434)
    x, dy = torch.randn(2, C, 34, 34, generator=g).to(DEV), torch.randn(2, C, 34, 34, generator=g).to(DEV)
    ys, dxs, gs = _run(mod, x, dy, True)
    yc, dxc, gc = _run(mod, x, dy, False)
    print(f"AttnBlock(512) 2x34x34: y rl2 {_rl2(ys, yc):.3e}  proj_out.weight.grad rl2 {_rl2(gs['proj_out.weight'], gc['proj_out.weight']):.3e}")
    assert _rl2(ys, yc) < 6e-3
    assert torch.equal(dxs, dxc)                    # dx and these gradients never read o, and P is recomputed by the calls the composed forward makes
    for n in gc:
        if n == "proj_out.weight":
            assert _rl2(gs[n], gc[n]) < 6e-3
        else:
            assert torch.equal(gs[n], gc[n]), n
    ys2, dxs2, gs2 = _run(mod, x, dy, True)
    assert torch.equal(ys, ys2) and torch.equal(dxs, dxs2) and all(torch.equal(gs[n], gs2[n]) for n in gs)


# ---- 5b. a token count that is no multiple of 32: the zero-row padding of the composed ops against independent references ---------------------------------------
def test_composed_probabilities_at_1156_tokens_are_masked_and_match_float64():
    """functional._attn_probs on operands padded from 1156 to 1184 rows: the padded keys' columns are EXACTLY zero in every row, the live block is float64's softmax
    to bf16 rounding (2^-9 relative per element, bar 2^-8 of the largest), the padded queries' rows are uniform over the live keys; P V on the padded v is
    float64's attention at the kernels' bars."""
    from dmvae_amd import functional as Fn, ops
    s, sp = 1156, 1184
    q, k, v = _randn_qkv(2, s, 1.5, 5150)
    p = Fn._attn_probs(Fn._attn_pad(q, sp), Fn._attn_pad(k, sp), SCALE, s)
    assert p.shape == (2, sp, sp) and p.dtype == BF
    assert (p[:, :, s:] == 0).all()                         # no weight on a padded key, in live and in padded rows
    ref_p = torch.softmax(q.double() @ k.double().transpose(-2, -1) * SCALE, dim=-1)
    perr = (p[:, :s, :s].double() - ref_p).abs().max().item()
    print(f"P at S={s}: max|err| {perr:.3e} (bar {2 ** -8 * ref_p.max().item():.3e})  rl2 {_rl2(p[:, :s, :s], ref_p):.3e}")
    assert perr < 2 ** -8 * ref_p.max().item() and _rl2(p[:, :s, :s], ref_p) < 6e-3
    assert (p[:, s:, :s].double() - 1.0 / s).abs().max().item() < 2 ** -8 / s
    o = ops.gemm_nt(p, ops.transpose_last2(Fn._attn_pad(v, sp)))[:, :s]
    ref, _ = _ref64(q, k, v)
    err = (o.double() - ref).abs().max().item()
    print(f"P V at S={s}: max|err| {err:.3e} (bar {_bar(ref):.3e})  rl2 {_rl2(o, ref):.3e}")
    assert err < _bar(ref) and _rl2(o, ref) < 6e-3


_ORACLE = {}


def _oracle_34(mod, x, dy, sites):
    """float64 AttnBlock of oracle/ref_cpu.py (GroupNorm, 1x1 convs, softmax attention, proj_out, residual; autograd) on the module's weights -> (y, dx, grads);
    sites: with bf16 rounding at the HIP path's storage sites, or none.  Computed once per kind and shared by the two routes."""
    from oracle import ref_cpu as R
    if sites not in _ORACLE:
        q = R.bf16_round if sites else None
        po = {n: t.detach().double().cpu().requires_grad_(True) for n, t in mod.named_parameters()}
        xo = x.double().cpu().requires_grad_(True)
        yo = R.attn_block(xo if q is None else q(xo), po, "", q)
        yo.backward(dy.double().cpu() if q is None else q(dy.double().cpu()))
        _ORACLE[sites] = (yo.detach(), xo.grad, {n: t.grad for n, t in po.items()})
    return _ORACLE[sites]


@pytest.mark.parametrize("route", [True, False], ids=["streaming", "composed"])
def test_attnblock_at_34x34_against_the_float64_oracle(route):
    """Either route at 1156 tokens (padded to 1184 in the composed ops) against an independent reference, at tests/test_gpu_modules.py's bars for AttnBlock (relative to
    the tensor's max-abs): 8e-3 against the oracle with bf16 rounding at the storage sites, 3e-2 against the oracle without.  The q / k weights are small enough for a
    nearly flat softmax (scaled scores of standard deviation ~0.5): 28 unmasked padded keys would take 2 % of every row's weight and move o, proj_out.weight.grad
    and the gradients behind v by that much."""
    from conftest import rel_err
    mod = _attn_block(5, qk_gain=0.7)
    g = torch.Generator().manual_seed(1156)
    x, dy = torch.randn(1, C, 34, 34, generator=g).to(DEV), torch.randn(1, C, 34, 34, generator=g).to(DEV)
    y, dx, gs = _run(mod, x, dy, route)
    exact = _oracle_34(mod, x, dy, False)[2]
    for sites, tol in ((True, 8e-3), (False, 3e-2)):
        yo, dxo, go = _oracle_34(mod, x, dy, sites)
        errs = {"y": rel_err(y.cpu(), yo), "dx": rel_err(dx.cpu(), dxo)}
        for n in go:
            if exact[n].abs().max() < 1e-4:    # analytically zero in float64 (the key bias shifts every score of a row alike): rounding noise wherever bf16 sites are.
                # Its scale is its twin's: k.bias.grad is the column sum of dK as q.bias.grad is of dQ, over the same bf16 dS; held to the same fraction of that max-abs
                twin = exact[n.replace("k.", "q.", 1)].abs().max().item()
                print(f"{n}: max |grad| {gs[n].abs().max().item():.2e} (exactly zero in float64; bar {tol:g} x max|{n.replace('k.', 'q.', 1)}.grad| = {tol * twin:.2e})")
                assert n.startswith("k.") and gs[n].abs().max().item() < tol * twin, n
                continue
            errs[n] = rel_err(gs[n].cpu(), go[n])
        print(f"AttnBlock(512) 34x34 {'streaming' if route else 'composed'} vs oracle {'with bf16 sites' if sites else 'float64'}: " +
              "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        for n, e in errs.items():
            assert e < tol, (n, e, tol)


# ---- 6. nothing S x S is written or saved -------------------------------------------------------------------------------------------------
def test_attnblock_forward_at_4096_tokens_allocates_less_than_one_score_tensor():
    mod = _attn_block(4)
    s, b = 4096, 2
    bound = s * s * 4                # ONE sample's f32 score tensor, 67 MB; the composed forward holds [b, s, s] in f32 and in bf16: 201 MB
    g = torch.Generator().manual_seed(64)
    warm = torch.randn(1, 34, 34, C, generator=g).to(BF).to(DEV)
    x = torch.randn(b, 64, 64, C, generator=g).to(BF).to(DEV)
    with torch.no_grad():
        mod.forward_nhwc(warm)       # packed weights and workspaces exist before the measurement
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y = mod.forward_nhwc(x)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    print(f"AttnBlock(512) {b}x64x64 forward, no graph: peak {peak / 2**20:.1f} MiB above the input (bound {bound / 2**20:.1f} MiB)")
    assert torch.isfinite(y.float()).all()
    assert peak < bound
    del y
    before = torch.cuda.memory_allocated()
    y = mod.forward_nhwc(x.requires_grad_(True))
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    print(f"with a graph: {held / 2**20:.1f} MiB held after the forward")
    assert held < bound              # no P saved for backward


# ---- 7. Decoder and VAE at another resolution -------------------------------------------------------------------------------------------
def test_decoder_takes_324_tokens_like_an_18x18_latent_and_streams(monkeypatch):
    from dmvae_amd.models.flux_ae import Decoder
    torch.manual_seed(7)
    z = 32
    dec = Decoder(ch=128, out_ch=3, ch_mult=(1, 2, 4), num_res_blocks=1, in_channels=3, resolution=144, z_channels=z)      # mid block at 4 * 128 = 512 channels
    dec.post_init(z_channels=z)      # as VAE builds it: the latent grid is upsampled x2 ahead of the mid block, 18 x 18 -> 36 x 36 = 1296 tokens
    dec = dec.to(DEV).eval()
    calls = _count_calls(monkeypatch, "attention_wide_stream")
    tokens = torch.randn(2, 324, z, generator=torch.Generator().manual_seed(324)).to(DEV)
    with torch.no_grad():
        y_tok = dec(tokens)
        y_img = dec(tokens.transpose(1, 2).reshape(2, z, 18, 18).contiguous())
    assert len(calls) == 2
    assert y_tok.shape == (2, 3, 144, 144) and torch.isfinite(y_tok).all()
    assert torch.equal(y_tok, y_img)


def test_vae_runs_end_to_end_at_288_px():
    from dmvae_amd.models.vae import VAE
    torch.manual_seed(288)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = VAE(z_channels=32, model_size="base", encoder_kwargs=dict(embed_dim=256, depth=1, num_heads=4, img_size=288)).to(DEV)
    x = torch.randn(1, 3, 288, 288, generator=torch.Generator().manual_seed(1)).clamp_(-1, 1).to(DEV)

    def step():
        vae.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF):
            y = vae(x)
        assert y.shape == (1, 3, 288, 288) and y.dtype == torch.float32 and torch.isfinite(y).all()
        y.square().mean().backward()
        for n, p in vae.named_parameters():
            assert not p.requires_grad or (p.grad is not None and torch.isfinite(p.grad).all()), n
        grads = {n: p.grad.clone() for n, p in vae.named_parameters() if p.requires_grad}
        return y.detach(), grads

    y1, g1 = step()
    y2, g2 = step()
    assert torch.equal(y1, y2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    with torch.autocast("cuda", dtype=BF):
        img = vae.decode_uint8(vae.encode(x))
    assert img.shape == (1, 288, 288, 3) and img.dtype == torch.uint8
