"""The DINOv2 discriminator (reference: models/dinodisc.py + models/dinov2.py) restated on the CPU over plain parameter dicts, with bf16 rounding at exactly
the sites where the HIP route stores bf16 -- the twin the GPU tests measure that route against (rel-L2 to the f32 capture no more than
1.15 x the twin's).  `q=None`: plain f32, the module's definition, written with the torch operations the reference's modules call (F.layer_norm, Tensor.var, W / sigma): LeakyReLU's
derivative jumps at zero, so an f32 restatement that rounds a pre-activation differently can take the other side for one of 1.5 M elements, and that one element
moves single entries of a weight or image gradient by 3e-4 ... 3e-3 of the tensor's largest -- measured with a hand-written LayerNorm / variance in this file.  A helper module for tests/test_dinodisc_cpu.py and tests/test_gpu_dinodisc.py; also holds
the name-seeded fill the capture tool (tools/capture_golden_dinodisc.py) and the tests share.

bf16 sites (q = oracle.ref_cpu.bf16_round: value forward, gradient backward; weights: bf16_round_weight):
  backbone   as oracle.ref_cpu.vit_forward_features: every Linear's input, weight and result (the patch embedding included); f32 residual stream, LayerNorm,
             softmax and LayerScale
  tap        act = q(t[:, 1:] + t[:, :1])
  convs      weight pack q_w(W / sigma) (f32 division), f32 bias, result q(.)     [both C -> C convolutions]
  norms      statistics and normalisation in f32 on the stored bf16 tensor, LeakyReLU, result q(.)
  tail       logit = <(a + h) / sqrt 2, W2 / sigma2> + b2 in f32 on the stored a, h: no rounding
Spectral norm is f32 everywhere (one power iteration in train mode, v then u, eps 1e-12; sigma = u . (W v), differentiable through W only)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from oracle.detweights import det_tensor

PATCH = 14
SMALL = dict(ks=9, key_depths=(1, 3), depth=4, batch=12, px=256, seed=31, x_seed=5, dy_seed=6)      # tests/golden/dinodisc_small.npz


def filled_heads(shapes: dict, seed: int) -> dict:
    """Name-seeded values for a DinoDisc state_dict's head entries (`shapes`: key -> shape): det_tensor, norm scales moved to 1 + 2 x, then every weight_u /
    weight_v normalised -- what the capture tool loads into the reference's module and the tests into this build's."""
    out = {}
    for k, shp in shapes.items():
        if not k.startswith("heads."):
            continue
        v = det_tensor(k, tuple(shp), seed)
        if k.endswith(".1.weight"):                       # the norm's scale (heads.i.0.1 / heads.i.1.fn.1)
            v = 1.0 + 2.0 * v
        if k.endswith("weight_u") or k.endswith("weight_v"):
            v = F.normalize(v, dim=0, eps=1e-12)
        out[k] = v
    return out


def filled_backbone(shapes: dict, seed: int) -> dict:
    return {k: det_tensor(k, tuple(shp), seed) for k, shp in shapes.items()}


def image(batch: int, px: int, seed: int) -> torch.Tensor:
    return torch.rand(batch, 3, px, px, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def pos_embed_for(pos: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """models/dinov2.py:179-211 (interpolate_offset 0.1, no antialias)."""
    n = pos.shape[1] - 1
    h0, w0 = h // PATCH, w // PATCH
    if h0 * w0 == n and h == w:
        return pos
    m = int(math.sqrt(n))
    g = F.interpolate(pos[:, 1:].reshape(1, m, m, -1).permute(0, 3, 1, 2), mode="bicubic", antialias=False, scale_factor=((h0 + 0.1) / m, (w0 + 0.1) / m))
    return torch.cat([pos[:, :1], g.permute(0, 2, 3, 1).reshape(1, h0 * w0, -1)], dim=1)


def preprocess(x, branch, crop=None):
    """models/dinodisc.py:166-178 with the branch named by the caller: 'area', 'crop' (offsets given) or 'bicubic'."""
    mean, std = torch.tensor((0.485, 0.456, 0.406)), torch.tensor((0.229, 0.224, 0.225))
    x = x if x.dtype == torch.float64 else x.float()          # (float64 in, float64 through: the f32 constants are the module's buffers)
    x = (0.5 / std).reshape(1, 3, 1, 1).to(x.dtype) * x + ((0.5 - mean) / std).reshape(1, 3, 1, 1).to(x.dtype)
    h, w = x.shape[-2:]
    nh, nw = h // PATCH * PATCH, w // PATCH * PATCH
    if branch == "crop":
        return x[..., crop[0]:crop[0] + nh, crop[1]:crop[1] + nw]
    return F.interpolate(x, size=(nh, nw), mode="area" if branch == "area" else "bicubic")


def backbone_taps(x, p, key_depths, num_heads, q=None):
    """The un-normed residual stream after the blocks in key_depths (models/dinov2.py:213-232,272-282; block algebra dino_layers/block.py:89-115)."""
    t = F.conv2d(R._q(q, x), R._qw(q, p["patch_embed.proj.weight"]), p["patch_embed.proj.bias"], stride=PATCH)
    b, c = t.shape[:2]
    t = R._q(q, t.flatten(2).transpose(1, 2))
    t = torch.cat([p["cls_token"].expand(b, -1, -1), t], dim=1) + pos_embed_for(p["pos_embed"], x.shape[-2], x.shape[-1])
    hd = c // num_heads
    taps = []
    for i in range(max(key_depths) + 1):
        bp = f"blocks.{i}."
        h = F.layer_norm(t, (c,), p[bp + "norm1.weight"], p[bp + "norm1.bias"], 1e-6)
        qkv = R.linear(h, p, bp + "attn.qkv", q).reshape(b, -1, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
        att = torch.softmax((qkv[0] * hd ** -0.5) @ qkv[1].transpose(-2, -1), dim=-1)
        h = R.linear((att @ qkv[2]).transpose(1, 2).reshape(b, -1, c), p, bp + "attn.proj", q)
        t = t + h * p[bp + "ls1.gamma"]
        h = F.layer_norm(t, (c,), p[bp + "norm2.weight"], p[bp + "norm2.bias"], 1e-6)
        h = R.linear(F.gelu(R.linear(h, p, bp + "mlp.fc1", q)), p, bp + "mlp.fc2", q)
        t = t + h * p[bp + "ls2.gamma"]
        if i in key_depths:
            taps.append(t)
    return taps


def sigma_of(p, pre, train):
    """-> (sigma [1], u, v): torch's legacy SpectralNorm (dim 0, one power iteration in train mode, eps 1e-12); u, v are the buffers after the call."""
    w = p[pre + "weight_orig"]
    wm = w.reshape(w.shape[0], -1)
    u, v = p[pre + "weight_u"], p[pre + "weight_v"]
    if train:
        with torch.no_grad():
            v = F.normalize(torch.mv(wm.t(), u), dim=0, eps=1e-12)
            u = F.normalize(torch.mv(wm, v), dim=0, eps=1e-12)
    return torch.dot(u, torch.mv(wm, v)).reshape(1), u, v


def batchnorm_local(x, w, b, eps=1e-6, virtual_bs=8):
    """models/dinodisc.py:40-56 on [B, C, L]."""
    g = int(np.ceil(x.shape[0] / virtual_bs))
    xg = x.reshape(g, -1, x.shape[-2], x.shape[-1])
    mean = xg.mean([1, 3], keepdim=True)
    var = xg.var([1, 3], keepdim=True, unbiased=False)
    return ((xg - mean) / torch.sqrt(var + eps) * w[None, :, None] + b[None, :, None]).reshape(x.shape)


def head(t, p, pre, ks, train, q=None, new_uv=None):
    """One head on the tap t [B, 1 + L, C] -> logits [B, L] (models/dinodisc.py:134-141,182-190)."""
    act = R._q(q, t[:, 1:] + t[:, :1]).transpose(1, 2)                         # [B, C, L]

    def conv_w(cpre):
        s, u, v = sigma_of(p, cpre, train)
        if new_uv is not None:
            new_uv[cpre + "weight_u"], new_uv[cpre + "weight_v"] = u, v
        return p[cpre + "weight_orig"] / s

    h0 = R._q(q, F.conv1d(act, R._qw(q, conv_w(pre + "0.0.")), p[pre + "0.0.bias"]))
    a = R._q(q, F.leaky_relu(batchnorm_local(h0, p[pre + "0.1.weight"], p[pre + "0.1.bias"]), 0.2))
    c1 = R._q(q, F.conv1d(a, R._qw(q, conv_w(pre + "1.fn.0.")), p[pre + "1.fn.0.bias"], padding=ks // 2))
    h = R._q(q, F.leaky_relu(batchnorm_local(c1, p[pre + "1.fn.1.weight"], p[pre + "1.fn.1.bias"]), 0.2))
    return F.conv1d((a + h) * (1 / math.sqrt(2)), conv_w(pre + "2."), p[pre + "2.bias"]).reshape(t.shape[0], -1)


def forward(x, backbone, heads, ks, key_depths, num_heads=6, train=True, branch="area", crop=None, q=None, new_uv=None):
    """Logits [B, len(key_depths) * L] from an image in [-1, 1]; `backbone` / `heads`: parameter dicts under the reference's key names."""
    taps = backbone_taps(preprocess(x, branch, crop), backbone, key_depths, num_heads, q)
    return torch.cat([head(t, heads, f"heads.{i}.", ks, train, q, new_uv) for i, t in enumerate(taps)], dim=1)


def build_module(device="cpu", ks=SMALL["ks"], key_depths=SMALL["key_depths"], depth=SMALL["depth"], seed=SMALL["seed"], **kw):
    """This build's DinoDisc with the capture's reduced ViT-S backbone and name-seeded weights; -> (module, backbone dict, heads dict)."""
    import warnings
    from dmvae_amd.models.dinodisc import DinoDisc
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        disc = DinoDisc(ks, "cpu", None, key_depths=key_depths, dino_depth=depth, **kw)
    backbone = filled_backbone({k: v.shape for k, v in disc.dino[0].state_dict().items()}, seed)
    disc.dino[0].load_state_dict(backbone, strict=True)
    heads = filled_heads({k: v.shape for k, v in disc.state_dict().items()}, seed)
    missing, unexpected = disc.load_state_dict(heads, strict=False)
    assert set(missing) == {"x_scale", "x_shift"} and not unexpected
    return disc.to(device), backbone, heads
