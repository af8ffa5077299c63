"""csrc/attention_bwd_stream.hip (-m gpu): the encoder's attention backward beyond the 288 tokens the resident kernel holds in LDS -- a query pass (dQ, delta)
and a key pass (dK, dV) that stream 64-row tiles (reference: autograd of models/dino_layers/attention.py:56-69 at the token counts patch_size / img_size reach
through models/vae.py:38-50).

Bars are test_gpu_attention_bwd.py's, per component dq / dk / dv against float64 autograd on the same bf16 operands: rel-L2 < 1.2e-2, max-error / max < 3e-2, and
|.| < 1e-5 where the true gradient is identically zero.  The kernel rounds P and dS to bf16 where they enter the matrix cores, as the resident kernel and the
GEMM-composed route do; an emulation of exactly those rounding sites in f32 gives rel-L2 <= 3.5e-3 and max-error / max <= 7.1e-3 on the shapes of test 1 (6.9e-3
rel-L2 on the randn x 4 inputs of test 2), so the bars leave about 3x for the kernel's summation order.  Reruns and batch splits are bit-identical."""
import copy

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
D = 64
SCALE = D ** -0.5
RL2_BAR, REL_BAR, ZERO_BAR = 1.2e-2, 3e-2, 1e-5


def _rl2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _ref64(qkv, do, h):
    """qkv [B, S, 3*h*64], do [B, S, h*64] (bf16, on the GPU) -> float64 d(qkv) [B, S, 3, h*64] of softmax(scale q k^T) v by autograd on the same values."""
    b, s, _ = qkv.shape
    q, k, v = (qkv.double().view(b, s, 3, h, D)[:, :, i].permute(0, 2, 1, 3).clone().requires_grad_(True) for i in range(3))
    o = torch.softmax(SCALE * q @ k.transpose(-1, -2), dim=-1) @ v
    o.backward(do.double().view(b, s, h, D).permute(0, 2, 1, 3))
    return torch.stack([q.grad, k.grad, v.grad], 0).permute(1, 3, 0, 2, 4).reshape(b, s, 3, h * D)


_CASES = {}


def _case(b, s, h, mult=1.5, zero_q=False):
    """(qkv, do, float64 reference): computed once per shape and shared; nobody writes to them.  randn x mult in bf16, as the sibling tests use."""
    key = (b, s, h, mult, zero_q)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * s + 10 * h + b)
        qkv = torch.randn(b, s, 3, h, D, generator=g) * mult
        if zero_q:
            qkv[:, :, 0] = 0
        qkv = qkv.to(BF).to(DEV).view(b, s, 3 * h * D)
        do = torch.randn(b, s, h * D, generator=g).to(BF).to(DEV)
        _CASES[key] = (qkv, do, _ref64(qkv, do, h))
    return _CASES[key]


def _stream_bwd(qkv, do, h):
    """forward (out, lse) from the streaming forward, then the streaming backward through its direct entry"""
    from dmvae_amd import ops
    out, lse = ops.attention_qkv_stream(qkv, h, SCALE, need_lse=True)
    return ops.attention_bwd_qkv_stream(qkv, out, do, h, SCALE, lse), out, lse


def _hold(got, want, tag, zero=()):
    """got [B, S, 3*C] bf16 against want [B, S, 3, C] float64, per component; components named in `zero` have an identically zero true gradient"""
    b, s, _, c = want.shape
    assert got.shape == (b, s, 3 * c) and got.dtype == BF and torch.isfinite(got.float()).all(), tag
    errs = {}
    for i, name in enumerate(("dq", "dk", "dv")):
        g, w = got.view(b, s, 3, c)[:, :, i], want[:, :, i]
        if name in zero:
            assert w.abs().max().item() == 0.0, (tag, name)          # the input does what it is meant to
            print(f"{tag} {name}: max|.| {g.float().abs().max().item():.3e} (true gradient identically zero)")
            assert g.float().abs().max().item() < ZERO_BAR, (tag, name, g.float().abs().max().item())
            continue
        errs[name] = _rl2(g, w)
        print(f"{tag} {name}: rl2 {errs[name]:.3e}  rel_err {rel_err(g, w):.3e}")
        assert errs[name] < RL2_BAR, (tag, name, errs[name])
        assert rel_err(g, w) < REL_BAR, (tag, name, rel_err(g, w))
    return errs


# ---- 1. the kernels against float64 autograd, direct entry ---------------------------------------------------------------------------
@pytest.mark.parametrize("b,s,h", [(1, 1, 2),        # a single key: the softmax is constant, dq = dk = 0
                                   (2, 17, 3),       # less than one tile
                                   (1, 64, 1),       # exactly one tile
                                   (1, 65, 2),       # one live key in the second tile
                                   (1, 257, 2),      # one live query in the second query block (and one live key in the second key block)
                                   (1, 289, 2),      # first length over the resident cap
                                   (2, 325, 4),
                                   (1, 577, 2),      # 384 px at patch 16
                                   (1, 1025, 1)])    # patch 8 at 256 px
def test_stream_backward_vs_float64(b, s, h):
    qkv, do, want = _case(b, s, h)
    got, _, _ = _stream_bwd(qkv, do, h)
    _hold(got, want, f"attention_bwd_qkv_stream {b}x{s}x{h}", zero=("dq", "dk") if s == 1 else ())
    assert torch.equal(got, _stream_bwd(qkv, do, h)[0])          # fixed summation order


# ---- 2. harder inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [289, 577])
@pytest.mark.parametrize("kind", ["randn4", "zeroq"])
def test_stream_backward_hard_inputs(s, kind):
    """randn x 4: near-one-hot probability rows (large, cancelling dP - delta); q = 0: uniform P, and dk = scale dS^T Q is identically zero."""
    h = 2
    qkv, do, want = _case(1, s, h, mult=4.0) if kind == "randn4" else _case(1, s, h, zero_q=True)
    got, _, _ = _stream_bwd(qkv, do, h)
    _hold(got, want, f"{kind} S={s}", zero=("dk",) if kind == "zeroq" else ())


# ---- 3. no further from float64 than the composed route --------------------------------------------------------------------------------
@pytest.mark.parametrize("b,s,h", [(2, 325, 4), (1, 577, 2)])
def test_stream_backward_twin_of_the_composed_route(b, s, h):
    from dmvae_amd import functional as Fn
    qkv, do, want = _case(b, s, h)
    got, _, _ = _stream_bwd(qkv, do, h)
    comp = Fn._attention_bwd(qkv, do, h, SCALE)
    c = h * D
    for i, name in enumerate(("dq", "dk", "dv")):
        e_stream = _rl2(got.view(b, s, 3, c)[:, :, i], want[:, :, i])
        e_comp = _rl2(comp.view(b, s, 3, c)[:, :, i], want[:, :, i])
        print(f"S={s} {name}: streaming {e_stream:.3e}  composed {e_comp:.3e}")
        assert e_stream < 1.5 * e_comp + 5e-3, (name, e_stream, e_comp)


# ---- 4. agreement with the resident kernel where both apply --------------------------------------------------------------------------
@pytest.mark.parametrize("s", [200, 288])
def test_stream_backward_agrees_with_the_resident_kernel(s):
    from dmvae_amd import ops
    b, h = 2, 2
    qkv, do, _ = _case(b, s, h)
    out, lse = ops.attention_qkv(qkv, h, SCALE, need_lse=True)              # the resident forward
    res = ops.attention_bwd_qkv(qkv, out, do, h, SCALE, lse=lse)
    st = ops.attention_bwd_qkv_stream(qkv, out, do, h, SCALE, lse)
    c = h * D
    for i, name in enumerate(("dq", "dk", "dv")):
        e = _rl2(st.view(b, s, 3, c)[:, :, i], res.view(b, s, 3, c)[:, :, i])
        print(f"S={s} {name}: streaming vs resident rl2 {e:.3e}")
        assert e < RL2_BAR, (name, e)


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------
def test_stream_backward_batch_split_is_bit_identical():
    from dmvae_amd import ops
    h, s = 2, 325
    qkv, do, _ = _case(4, s, h)
    out, lse = ops.attention_qkv_stream(qkv, h, SCALE, need_lse=True)
    full = ops.attention_bwd_qkv_stream(qkv, out, do, h, SCALE, lse)
    assert torch.equal(full, ops.attention_bwd_qkv_stream(qkv, out, do, h, SCALE, lse))
    halves = [ops.attention_bwd_qkv_stream(qkv[i:i + 2].contiguous(), out[i:i + 2].contiguous(), do[i:i + 2].contiguous(), h, SCALE,
                                           lse[i * h:(i + 2) * h].contiguous()) for i in (0, 2)]
    assert torch.equal(full, torch.cat(halves))


# ---- 6. dispatch -----------------------------------------------------------------------------------------------------------------------
def test_dispatch_keeps_the_resident_backward_up_to_288_tokens_and_streams_above():
    from dmvae_amd import ops, _lib
    b, h = 2, 2
    qkv, do, _ = _case(b, 288, h)
    out, lse = ops.attention_qkv(qkv, h, SCALE, need_lse=True)
    want = torch.empty_like(qkv)      # dmvae_attention_bwd_qkv_lse_bf16 called through the C ABI, not through ops.attention_bwd_qkv
    ops.check(_lib.lib().dmvae_attention_bwd_qkv_lse_bf16(qkv.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(), want.data_ptr(), b, 288, h, D, float(SCALE),
                                                          ops._stream()), "attention_bwd_qkv_bf16")
    assert torch.equal(ops.attention_bwd_qkv(qkv, out, do, h, SCALE, lse=lse), want)
    qkv, do, _ = _case(1, 289, h)
    out, lse = ops.attention_qkv(qkv, h, SCALE, need_lse=True)
    assert torch.equal(ops.attention_bwd_qkv(qkv, out, do, h, SCALE, lse=lse), ops.attention_bwd_qkv_stream(qkv, out, do, h, SCALE, lse))
    with pytest.raises(ValueError):
        ops.attention_bwd_qkv(qkv, out, do, h, SCALE)                       # above the cap the row statistics are required
    with pytest.raises(ValueError):
        ops.attention_bwd_qkv_stream(qkv, out, do, h, SCALE, None)


# ---- 7. through the trainable encoder --------------------------------------------------------------------------------------------------
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


def test_trainable_encoder_at_325_tokens_never_takes_the_composed_backward(monkeypatch):
    """288 px / patch 16 = 325 tokens, B = 2, with `functional._attention_bwd` made to raise: forward and backward complete on the kernels, with finite gradients for
    the input and every parameter, bit-identical over two runs.  Then, un-patched, the gradients against the stock module under autocast(bf16): 3e-2 rel-L2 each, and
    against the f32 stock gradients no further away than the stock bf16 twin measured in the same run (e_hip < 1.5 e_stock + 5e-3)."""
    from dmvae_amd import functional as Fn
    from dmvae_amd.models import vit_fast
    vit = _vit(256, 2, 4, 288)
    ref = copy.deepcopy(vit)
    assert vit.pos_embed.shape[1] == 325 and vit_fast.hip_path_supported(vit, 325)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 288, 288, generator=g).to(DEV)
    dy = torch.randn(2, 325, 256, generator=g).to(DEV)

    def hip_run():
        vit.zero_grad(set_to_none=True)
        xa = x.clone().requires_grad_(True)
        ya = vit.forward_features(xa)                                   # trainable, CUDA, supported width: the HIP route
        assert ya.dtype == BF and ya.shape == (2, 325, 256)
        (ya.float() * dy).sum().backward()
        assert xa.grad is not None and all(p.grad is not None for p in vit.parameters())
        return ya, xa, [ya.detach().clone(), xa.grad.clone()] + [p.grad.clone() for p in vit.parameters()]

    def composed_route_is_gone(*args, **kwargs):
        raise AssertionError("the composed attention backward was called at head dim 64")

    with monkeypatch.context() as m:
        m.setattr(Fn, "_attention_bwd", composed_route_is_gone)
        runs = [hip_run()[2] for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)

    ya, xa, _ = hip_run()
    ref32 = copy.deepcopy(ref)
    # the stock twins' patch embedding is an nn.Conv2d: with the vendor convolution library switched off ATen runs it as an unfold + GEMM, the same sums, instead
    # of a per-shape kernel search on the first backward call at this image size; the route under test has no convolution (one GEMM over patches)
    with torch.backends.cudnn.flags(enabled=False):
        xb = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=BF):
            yb = ref.forward_features_stock(xb)
            (yb.float() * dy).sum().backward()
        xc = x.clone().requires_grad_(True)
        yc = ref32.forward_features_stock(xc)
        (yc * dy).sum().backward()
    pa, pb, p32 = dict(vit.named_parameters()), dict(ref.named_parameters()), dict(ref32.named_parameters())
    e_hip = max(_rl2(pa[n].grad, p32[n].grad) for n in pa)
    e_stock = max(_rl2(pb[n].grad, p32[n].grad) for n in pa)
    print(f"325 tokens: dx hip/stock-bf16 {_rl2(xa.grad, xb.grad):.3e}  param grads vs f32: hip {e_hip:.3e}  stock-bf16 {e_stock:.3e};  dx vs f32: hip "
          f"{_rl2(xa.grad, xc.grad):.3e}  stock-bf16 {_rl2(xb.grad, xc.grad):.3e}")
    assert _rl2(xa.grad, xb.grad) < 3e-2
    for n in pa:
        assert _rl2(pa[n].grad, pb[n].grad) < 3e-2, (n, _rl2(pa[n].grad, pb[n].grad))
    assert e_hip < 1.5 * e_stock + 5e-3, (e_hip, e_stock)


# ---- 8. memory -------------------------------------------------------------------------------------------------------------------------
def test_backward_above_the_cap_allocates_less_than_one_score_matrix():
    """One `ops.attention_bwd_qkv` call at 577 tokens: dqkv (1.8 MB) + delta (18 KB), against the b * h * s^2 * 4 bytes (10.7 MB) of ONE of the four S x S f32 tensors
    the composed route keeps."""
    from dmvae_amd import ops
    b, s, h = 2, 577, 4
    qkv, do, _ = _case(b, s, h)
    out, lse = ops.attention_qkv(qkv, h, SCALE, need_lse=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dqkv = ops.attention_bwd_qkv(qkv, out, do, h, SCALE, lse=lse)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"attention_bwd_qkv {b}x{s}x{h}: peak allocation {peak / 1e6:.2f} MB (one S x S f32 tensor: {b * h * s * s * 4 / 1e6:.2f} MB)")
    assert dqkv.shape == qkv.shape
    assert peak < b * h * s * s * 4, peak
