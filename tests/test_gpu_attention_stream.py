"""csrc/attention_stream.hip (-m gpu): the encoder's fused attention beyond the 288 tokens the resident kernel holds in LDS -- 64-key K / V tiles streamed
with an online softmax (reference: models/dino_layers/attention.py:56-69 at the token counts patch_size / img_size reach through models/vae.py:38-50).

Bars are the ones the resident kernel is held to: max|err| < 2e-2 max|ref| + 1e-3 (test_gpu_train_step.py), rel-L2 < 6e-3 and |lse - logsumexp| < 2e-3
(test_gpu_attention_bwd.py), all against float64 softmax attention on the same bf16 operands; reruns and batch splits bit-identical.  The hard inputs make
every tile raise the running maximum (the rescale of the accumulators is exercised on every step, not only on lucky data)."""
import copy
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
D = 64
SCALE = D ** -0.5


def _rl2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _ref64(qkv, h):
    """qkv [B, S, 3*h*64] bf16 -> float64 (out [B, S, h*64], lse [B*h, S]) of softmax(scale q k^T) v on the same values."""
    b, s, c3 = qkv.shape
    t = qkv.double().reshape(b, s, 3, h, D).permute(2, 0, 3, 1, 4)
    sc = t[0] @ t[1].transpose(-2, -1) * SCALE
    out = (torch.softmax(sc, dim=-1) @ t[2]).transpose(1, 2).reshape(b, s, h * D)
    return out, torch.logsumexp(sc, dim=-1).reshape(b * h, s)


def _bar(ref):
    return 2e-2 * ref.abs().max().item() + 1e-3


def _check(fn, qkv, h, tag):
    """fn(qkv, h, SCALE, need_lse=True) against float64 at the resident kernel's bars; second call bit-identical.  Returns (out, lse, ref)."""
    out, lse = fn(qkv, h, SCALE, need_lse=True)
    ref, lse_ref = _ref64(qkv, h)
    assert out.shape == ref.shape and out.dtype == BF and lse.shape == lse_ref.shape and lse.dtype == torch.float32
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), tag
    err, rl2, lerr = (out.double() - ref).abs().max().item(), _rl2(out, ref), (lse.double() - lse_ref).abs().max().item()
    print(f"{tag}: max|err| {err:.3e} (bar {_bar(ref):.3e})  rl2 {rl2:.3e}  lse err {lerr:.3e}")
    assert err < _bar(ref), (tag, err)
    assert rl2 < 6e-3, (tag, rl2)
    assert lerr < 2e-3, (tag, lerr)
    out2, lse2 = fn(qkv, h, SCALE, need_lse=True)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), tag
    assert torch.equal(fn(qkv, h, SCALE), out), tag + ": the form without lse"
    return out, lse, ref


def _randn_qkv(b, s, h, mult, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, s, 3 * h * D, generator=g) * mult).to(BF).to(DEV)


# ---- 1. the kernel against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,s,h", [(1, 289, 2),      # first length over the cap: one live query in the last query block, one live key in the last tile
                                   (1, 320, 1),      # a multiple of 32 and 64: no masking
                                   (2, 577, 2),      # several tiles, ragged (384 px at patch 16)
                                   (1, 1025, 2)])    # the target shape (patch 8 at 256 px)
def test_stream_attention_vs_float64_through_dispatch(b, s, h):
    from dmvae_amd import ops
    _check(ops.attention_qkv, _randn_qkv(b, s, h, 1.5, 1000 * s + h), h, f"attention_qkv {b}x{s}x{h}")


@pytest.mark.parametrize("b,s,h", [(2, 17, 3),       # less than one tile
                                   (1, 1, 2),        # a single key
                                   (1, 64, 1)])      # exactly one tile
def test_stream_attention_vs_float64_direct_short(b, s, h):
    from dmvae_amd import ops
    _check(ops.attention_qkv_stream, _randn_qkv(b, s, h, 1.5, 1000 * s + h), h, f"attention_qkv_stream {b}x{s}x{h}")


# ---- 2. inputs that force the rescale on every tile ------------------------------------------------------------------------------------
def _directed(s, h, kind, seed):
    """[1, s, 3*h*64] bf16.  Queries: g_i * u, g_i in [14, 16], one unit direction u per head.  Keys: coef_j * u -- 'ascending': coef rises linearly from 0 to 8
    over j (scaled scores up to 16, every 64-key tile raises the running maximum); 'last': the same coefficients x 0.2 except the last key = 8 u (scores <= 3.2,
    then 14 .. 16 on the very last key of the ragged last tile).  'zeroq': zero queries, random keys.  V: randn x 1.5."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(h, D, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    gq = 14 + 2 * torch.rand(s, h, 1, generator=g)
    q = gq * u
    coef = torch.linspace(0, 8, s).view(s, 1, 1)
    if kind == "last":
        coef = coef * 0.2
        coef[-1] = 8.0
    k = coef * u
    if kind == "zeroq":
        q = torch.zeros(s, h, D)
        k = torch.randn(s, h, D, generator=g) * 1.5
    v = torch.randn(s, h, D, generator=g) * 1.5
    return torch.stack([q, k, v], dim=1).reshape(1, s, 3 * h * D).to(BF).to(DEV)


@pytest.mark.parametrize("s", [289, 577])
@pytest.mark.parametrize("kind", ["ascending", "last", "zeroq", "randn4"])
def test_stream_attention_rescale_inputs(s, kind):
    from dmvae_amd import ops
    h = 2
    qkv = _randn_qkv(1, s, h, 4.0, s + 7) if kind == "randn4" else _directed(s, h, kind, s + len(kind))
    out, lse, ref = _check(ops.attention_qkv_stream, qkv, h, f"{kind} S={s}")
    v = qkv.view(1, s, 3, h * D)[:, :, 2].double()
    if kind == "last":          # the last key takes (nearly) all the weight: every output row is V[S - 1]
        assert (ref - v[:, -1:]).abs().max().item() < _bar(ref)       # the inputs do what they are meant to
        assert (out.double() - v[:, -1:]).abs().max().item() < _bar(ref)
    if kind == "zeroq":         # uniform weights: every output row is the mean of V
        assert (out.double() - v.mean(dim=1, keepdim=True)).abs().max().item() < _bar(ref)


# ---- 3. batch independence -----------------------------------------------------------------------------------------------------------
def test_stream_attention_batch_split_is_bit_identical():
    from dmvae_amd import ops
    h = 2
    qkv = _randn_qkv(4, 325, h, 1.5, 325)
    out, lse = ops.attention_qkv_stream(qkv, h, SCALE, need_lse=True)
    o0, l0 = ops.attention_qkv_stream(qkv[:2].contiguous(), h, SCALE, need_lse=True)
    o1, l1 = ops.attention_qkv_stream(qkv[2:].contiguous(), h, SCALE, need_lse=True)
    assert torch.equal(out, torch.cat([o0, o1])) and torch.equal(lse, torch.cat([l0, l1]))


# ---- 4. dispatch -----------------------------------------------------------------------------------------------------------------------
def _resident_direct(qkv, h):
    """dmvae_attention_qkv_lse_bf16 called through the C ABI, not through ops.attention_qkv"""
    from dmvae_amd import ops, _lib
    b, s, c3 = qkv.shape
    out = torch.empty(b, s, c3 // 3, dtype=BF, device=qkv.device)
    lse = torch.empty(b * h, s, dtype=torch.float32, device=qkv.device)
    ops.check(_lib.lib().dmvae_attention_qkv_lse_bf16(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), b, s, h, D, float(SCALE), ops._stream()), "attention_qkv_bf16")
    return out, lse


def test_dispatch_keeps_the_resident_kernel_up_to_288_tokens_and_streams_above():
    from dmvae_amd import ops
    h = 3
    for s in (257, 288):
        qkv = _randn_qkv(2, s, h, 1.5, s)
        want, want_lse = _resident_direct(qkv, h)
        got, got_lse = ops.attention_qkv(qkv, h, SCALE, need_lse=True)
        assert torch.equal(got, want) and torch.equal(got_lse, want_lse), s
        assert torch.equal(ops.attention_qkv(qkv, h, SCALE), want), s
    qkv = _randn_qkv(2, 289, h, 1.5, 289)
    a, a_lse = ops.attention_qkv(qkv, h, SCALE, need_lse=True)
    b_, b_lse = ops.attention_qkv_stream(qkv, h, SCALE, need_lse=True)
    assert torch.equal(a, b_) and torch.equal(a_lse, b_lse)
    assert torch.equal(ops.attention_qkv(qkv, h, SCALE), b_)
    # the two kernels on the same operands: different tilings of the same softmax
    qkv = _randn_qkv(2, 257, h, 1.5, 257)
    res, res_lse = _resident_direct(qkv, h)
    st, st_lse = ops.attention_qkv_stream(qkv, h, SCALE, need_lse=True)
    assert _rl2(st, res) < 6e-3, _rl2(st, res)
    assert (st_lse - res_lse).abs().max().item() < 2e-3


# ---- 5. frozen encoder above the cap ------------------------------------------------------------------------------------------------
def test_frozen_encoder_at_1025_tokens_runs_on_the_hip_route(monkeypatch):
    """patch 8 at 256 px = 1025 tokens, no opt-in to the stock route: the fused inference route, against the stock module under autocast(bf16) at the bar
    test_gpu_train_step.py holds the 17-token encoder to."""
    from dmvae_amd.models.vit import DinoV2ViT
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    torch.manual_seed(0)
    vit = DinoV2ViT(embed_dim=256, depth=2, num_heads=4, patch_size=8, img_size=256).to(DEV).eval()
    with torch.no_grad():
        for blk in vit.blocks:
            blk.ls1.gamma.fill_(0.5); blk.ls2.gamma.fill_(0.5)
    img = torch.randn(2, 3, 256, 256, generator=torch.Generator().manual_seed(4)).to(DEV)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            got = vit.forward_features(img)
    assert not [str(w.message) for w in caught if "dmvae" in str(w.filename) or "STOCK" in str(w.message)], [str(w.message) for w in caught]
    assert got.dtype == BF and got.shape == (2, 1025, 256)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        want = vit.forward_features_stock(img).float()
    rel = ((got.float() - want).norm() / want.norm()).item()
    print(f"frozen encoder 1025 tokens: relative norm vs stock autocast {rel:.3e}")
    assert rel < 2e-2, rel


def test_vae_encode_with_patch_8(monkeypatch):
    from dmvae_amd.models.vae import VAE
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    torch.manual_seed(5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "pretrained weights are not available offline"
        vae = VAE(z_channels=32, model_size="base", encoder_kwargs=dict(embed_dim=256, depth=1, num_heads=4), patch_size=8).to(DEV).eval()
    x = (torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    with torch.autocast("cuda", dtype=BF):
        z = vae.encode(x)
    assert z.shape == (2, 1024, 32) and torch.isfinite(z.float()).all() and z.float().abs().max() > 0


# ---- 6. trainable encoder above the cap -----------------------------------------------------------------------------------------------
def _vit(embed_dim, depth, heads, img, seed=0):
    """test_gpu_vit_train.py's recipe: LayerScale at O(1) so that both branches matter; non-trivial norms / biases; larger Linear weights"""
    from dmvae_amd.models.vit import DinoV2ViT
    torch.manual_seed(seed)
    vit = DinoV2ViT(embed_dim=embed_dim, depth=depth, num_heads=heads, patch_size=16, img_size=img).to(DEV)
    with torch.no_grad():
        for blk in vit.blocks:
            blk.ls1.gamma.uniform_(0.5, 1.5); blk.ls2.gamma.uniform_(0.5, 1.5)
        for n, p in vit.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.1)
            if "norm" in n and n.endswith("weight"):
                p.uniform_(0.7, 1.3)
            if n.endswith("fc1.weight") or n.endswith("fc2.weight") or n.endswith("qkv.weight") or n.endswith("proj.weight"):
                p.mul_(2.5)
        vit.cls_token.normal_(0, 0.5)
        vit.pos_embed.normal_(0, 0.5)
    return vit


def test_trainable_encoder_at_325_tokens_matches_stock_autocast():
    """test_gpu_vit_train.py::test_trainable_encoder_matches_stock_autocast at 288 px / patch 16 = 325 tokens, B = 2: the forward attention is the streaming
    kernel, its backward the composed route (`functional._attention_bwd`).  Tokens, input gradient and every parameter gradient against the stock module
    under autocast(bf16); the deciding assertion is that test's last one -- against the f32 stock gradients the HIP route is no further away than the stock bf16
    twin measured in the same run (e_hip < 1.5 e_stock + 5e-3).  A second run gives bit-identical gradients."""
    from dmvae_amd.models import vit_fast
    vit = _vit(256, 2, 4, 288)
    ref = copy.deepcopy(vit)
    assert vit.pos_embed.shape[1] == 325 and vit_fast.hip_path_supported(vit, 325)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 288, 288, generator=g).to(DEV)
    dy = torch.randn(2, 325, 256, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        vit.zero_grad(set_to_none=True)
        xa = x.clone().requires_grad_(True)
        ya = vit.forward_features(xa)                                   # trainable, CUDA, supported width: the HIP route
        assert ya.dtype == BF and ya.shape == (2, 325, 256)
        (ya.float() * dy).sum().backward()
        runs.append([ya.detach().clone(), xa.grad.clone()] + [p.grad.clone() for p in vit.parameters()])
    for a, b in zip(*runs):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    ref32 = copy.deepcopy(ref)
    # the stock twins' patch embedding is an nn.Conv2d: with the vendor convolution library switched off ATen runs it as an unfold + GEMM, the same sums, instead
    # of a per-shape kernel search on the first backward call at this image size (a minute); the route under test has no convolution (one GEMM over patches)
    with torch.backends.cudnn.flags(enabled=False):
        xb = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            yb = ref.forward_features_stock(xb)
            (yb.float() * dy).sum().backward()
        xc = x.clone().requires_grad_(True)
        yc = ref32.forward_features_stock(xc)
        (yc * dy).sum().backward()
    pa, pb = dict(vit.named_parameters()), dict(ref.named_parameters())
    p32 = dict(ref32.named_parameters())
    worst = max(pa, key=lambda n: _rl2(pa[n].grad, pb[n].grad))
    e_hip = max(_rl2(pa[n].grad, p32[n].grad) for n in pa)
    e_stock = max(_rl2(pb[n].grad, p32[n].grad) for n in pa)
    print(f"325 tokens: tokens hip/stock-bf16 {_rl2(ya.float(), yb.float()):.3e}  dx {_rl2(xa.grad, xb.grad):.3e}  worst param grad {worst} "
          f"{_rl2(pa[worst].grad, pb[worst].grad):.3e}")
    print(f"325 tokens: stock-bf16 vs f32: tokens {_rl2(yb.float(), yc):.3e}  dx {_rl2(xb.grad, xc.grad):.3e}  params (max) {e_stock:.3e};  hip vs f32: tokens "
          f"{_rl2(ya.float(), yc):.3e}  dx {_rl2(xa.grad, xc.grad):.3e}  params (max) {e_hip:.3e}")
    assert _rl2(ya.float(), yb.float()) < 1e-2
    assert _rl2(xa.grad, xb.grad) < 3e-2
    for n in pa:
        assert pa[n].grad is not None, n
        assert _rl2(pa[n].grad, pb[n].grad) < 3e-2, (n, _rl2(pa[n].grad, pb[n].grad))
    assert e_hip < 1.5 * e_stock + 5e-3, (e_hip, e_stock)


def test_composed_attention_backward_at_325_tokens_vs_float64():
    """The route the trainable encoder takes above 288 tokens (`functional._attention_bwd`) at test_gpu_attention_bwd.py's bar."""
    from dmvae_amd import functional as Fn
    b, s, h = 1, 325, 4
    c = h * D
    g = torch.Generator().manual_seed(s + h)
    qkv = (torch.randn(b, s, 3, h, D, generator=g) * 1.5).to(BF).to(DEV)
    do = torch.randn(b, s, c, generator=g).to(BF).to(DEV)
    q, k, v = (qkv[:, :, i].double().permute(0, 2, 1, 3).clone().requires_grad_(True) for i in range(3))
    o = torch.softmax(SCALE * q @ k.transpose(-1, -2), dim=-1) @ v
    o.backward(do.double().view(b, s, h, D).permute(0, 2, 1, 3))
    want = torch.stack([q.grad, k.grad, v.grad], 0).permute(1, 3, 0, 2, 4).reshape(b, s, 3 * c)
    got = Fn._attention_bwd(qkv.view(b, s, 3 * c), do, h, SCALE)
    assert got.shape == (b, s, 3 * c) and torch.isfinite(got.float()).all()
    for i, name in enumerate("qkv"):
        e = _rl2(got.view(b, s, 3, c)[:, :, i], want.view(b, s, 3, c)[:, :, i])
        assert e < 1.2e-2, (name, e)
