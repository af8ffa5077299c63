"""DinoDisc -- the DINOv2 discriminator the reference's trainers build with `--disc_type dino` (models/dinodisc.py; train_tokenizer.py:307-312, kernel size 9) --
with the reference's constructor arguments, forward signature and state_dict keys, on the HIP kernels.

A frozen DINOv2 ViT (patch 14, position embedding for 518 px interpolated to the input's grid) looks at the ImageNet-normalised image; after each block in
`key_depths` the UN-NORMED residual stream is tapped (patch tokens + class token) and fed to a small convolutional head over the token axis:

    SpectralConv1d(C, C, 1) -> norm -> LeakyReLU(0.2) -> ResidualBlock[ SpectralConv1d(C, C, ks) -> norm -> LeakyReLU(0.2) ] -> SpectralConv1d(C, 1, 1)

and the heads' logits are concatenated: [B, len(key_depths) * L].

Routes.  The HIP route runs when the input is a GPU tensor under autocast(bfloat16), the fp32 parity mode is off, the backbone's width is one the LayerNorm
kernels take with head dim 64 and at most 512 channels (the heads' norm kernels: ViT-S, the scripts' backbone, is; ViT-B / L are not): backbone on the frozen encoder route (graph-free `vit_fast.frozen_forward_features`
with taps when the image needs no gradient -- the discriminator's turn --, `VitBlockDxFn` per block when it does -- the generator's term), each head as one
`functional.DinoHeadFn` (csrc/conv_tokens.hip, the GroupNorm kernels, csrc/dinodisc.hip).  Anything else goes through `_stock.require_opt_in` to
`forward_stock`, the plain-PyTorch statement of the module below, which is also its definition on the CPU.

Norms.  Both trainers build the module with `norm_type=args.disc_norm`, default "sbn", and `use_specnorm=args.disc_specnorm`, default False
(train_tokenizer.py:48-49,307-314, train_dmd.py:50-51,389-396): `nn.SyncBatchNorm(C, eps)` per block (models/dinodisc.py:62-65; 'lbn' / 'hbn': over the local
machine's process group, `dist.new_local_machine_group`), the holder of weight, bias, running_mean, running_var and num_batches_tracked under the reference's
keys.  On the HIP route it is the GroupNorm kernels with one "image" of B * L rows and one channel per group, the statistics through
`models.patchgan._bn_stats` -- PatchGAN's BatchNorm rule: combined over the ranks, running estimates updated with momentum 0.1 and the unbiased variance, the
backward's two per-channel sums all-reduced -- in train mode, and `functional.DinoHeadEvalFn` in eval mode with frozen heads (the generator's term): the running
estimates folded into the convolutions' epilogues.  The mode is chosen by `norm.training or not norm.track_running_stats`, as `_bn_stats` does.  'bn'
(BatchNormLocal, the module's own default) and 'gn' are selected by no script unless it is told to.

What differs from the reference, on purpose:
  * Spectral norm is computed in f32.  Under autocast the reference's `torch.mv` / `torch.dot` inside the legacy SpectralNorm hook run in bf16; the captured
    fixtures (f32, CPU) and this module follow the f32 arithmetic.
  * The random crop's offsets are drawn as torchvision's `RandomCrop.get_params` draws them -- `torch.randint(0, h - th + 1, (1,))` then
    `torch.randint(0, w - tw + 1, (1,))` on the global CPU generator.  torchvision is not a dependency of this build, so that order is this module's
    statement of it: UNPINNED against the real package.
  * `init_params` of the reference writes its xavier values into the recomputed `weight` attribute, which the next forward overwrites: it has no effect, and
    `weight_orig` keeps Conv1d's default initialisation there and here (biases zero, norm affine ones / zeros).  Seeded-construction RNG parity is not attempted.
  * `grad_ckpt=True` gives the same numbers; on the HIP route the head Function already keeps only what its backward reads, so nothing is recomputed.
  * `norm_type` 'sbn' / 'lbn' / 'hbn' (the SyncBatchNorm variants, models/dinodisc.py:62-65) sit behind a module-level switch that is off by default: with it off
    the constructor raises NotImplementedError.  `enable_syncbn_heads()` turns it on; `run_on_mi355x.install_shadow(ref, dinodisc=True)`, `--hip-dinodisc` and
    DMVAE_HIP_DINODISC=1 do so, since the scripts pass 'sbn'.
"""
import math
import random
import warnings

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .vit import DinoV2ViT

_SYNCBN_HEADS = False


def enable_syncbn_heads(on: bool = True) -> bool:
    """Turn the SyncBatchNorm head variants (`norm_type` 'sbn' / 'lbn' / 'hbn') on or off for constructors that follow; returns the previous setting."""
    global _SYNCBN_HEADS
    was, _SYNCBN_HEADS = _SYNCBN_HEADS, bool(on)
    return was


_ARCH = {"vit_small": dict(embed_dim=384, depth=12, num_heads=6), "vit_base": dict(embed_dim=768, depth=12, num_heads=12),
         "vit_large": dict(embed_dim=1024, depth=24, num_heads=16)}


class DinoBackbone(DinoV2ViT):
    """`DinoV2ViT` as models/dinodisc.py:79-105 builds it: patch 14, img_size 518 (pos_embed [1, 1370, C]), LayerScale init 1.0, plus the `mask_token` the
    reference's checkpoints carry (unused in a forward without masks), so that such a checkpoint loads strictly."""
    interpolate_offset = 0.1

    def __init__(self, embed_dim, depth, num_heads, patch_size=14, img_size=518):
        super().__init__(embed_dim=embed_dim, depth=depth, num_heads=num_heads, patch_size=patch_size, img_size=img_size)
        self.patch_size = patch_size
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))
        with torch.no_grad():
            for blk in self.blocks:
                blk.ls1.gamma.fill_(1.0)
                blk.ls2.gamma.fill_(1.0)
        self._pos_cache = {}

    def pos_for(self, h: int, w: int) -> torch.Tensor:
        """Position embedding [1, 1 + (h // p) * (w // p), C] for an h x w input, as models/dinov2.py:179-211: bicubic, `scale_factor` with the 0.1 offset, f32.
        Computed once per (h, w) and kept until the parameter changes."""
        pe = self.pos_embed
        key = (h, w, pe.data_ptr(), pe._version, pe.device, pe.dtype)
        hit = self._pos_cache.get((h, w))
        if hit is not None and hit[0] == key:
            return hit[1]
        n = pe.shape[1] - 1
        h0, w0 = h // self.patch_size, w // self.patch_size
        if h0 * w0 == n and h == w:
            out = pe.detach()
        else:
            m = int(math.sqrt(n))
            assert n == m * m
            p = pe.detach().float()
            grid = F.interpolate(p[:, 1:].reshape(1, m, m, -1).permute(0, 3, 1, 2), mode="bicubic", antialias=False,
                                 scale_factor=(float(h0 + self.interpolate_offset) / m, float(w0 + self.interpolate_offset) / m))
            assert (h0, w0) == tuple(grid.shape[-2:])
            out = torch.cat([p[:, :1], grid.permute(0, 2, 3, 1).reshape(1, h0 * w0, -1)], dim=1).to(pe.dtype)
        self._pos_cache[(h, w)] = (key, out)
        return out

    def taps_stock(self, x: torch.Tensor, key_depths):
        """The un-normed residual stream after the blocks in `key_depths` (get_intermediate_layers(norm=False), models/dinov2.py:272-322), stock PyTorch."""
        t = self.patch_embed(x)
        t = torch.cat([self.cls_token.expand(t.shape[0], -1, -1).to(t.dtype), t], dim=1) + self.pos_for(x.shape[-2], x.shape[-1]).to(t.dtype)
        taps = []
        for i, blk in enumerate(self.blocks):
            t = blk(t)
            if i in key_depths:
                taps.append(t)
        assert len(taps) == len(key_depths), f"only {len(taps)} / {len(key_depths)} blocks found"
        return taps


class SpectralConv1d(nn.Module):
    """Conv1d under torch's legacy spectral-norm hook (models/dinodisc.py:23-26: n_power_iterations 1, dim 0, eps 1e-12), stated without the hook: parameters
    `bias`, `weight_orig`, buffers `weight_u`, `weight_v` -- the hook's state_dict keys, in its order."""
    eps = 1e-12

    def __init__(self, cin, cout, kernel_size, padding=0):
        super().__init__()
        ref = nn.Conv1d(cin, cout, kernel_size, padding=padding)           # Conv1d's default initialisation
        self.kernel_size, self.padding = kernel_size, padding
        self.bias = nn.Parameter(torch.zeros_like(ref.bias))
        self.weight_orig = nn.Parameter(ref.weight.detach().clone())
        wm = self.weight_orig.detach().reshape(cout, -1)
        self.register_buffer("weight_u", F.normalize(wm.new_empty(cout).normal_(0, 1), dim=0, eps=self.eps))
        self.register_buffer("weight_v", F.normalize(wm.new_empty(wm.shape[1]).normal_(0, 1), dim=0, eps=self.eps))

    def sigma(self) -> torch.Tensor:
        """sigma = u . (W v) as an f32 [1] tensor, differentiable through W only; in train mode after one power iteration that updates v then u in place."""
        with torch.autocast(self.weight_orig.device.type, enabled=False):
            wm = self.weight_orig.float().reshape(self.weight_orig.shape[0], -1)
            if self.training:
                with torch.no_grad():
                    self.weight_v.copy_(F.normalize(torch.mv(wm.t(), self.weight_u), dim=0, eps=self.eps))
                    self.weight_u.copy_(F.normalize(torch.mv(wm, self.weight_v), dim=0, eps=self.eps))
            u, v = self.weight_u.clone(), self.weight_v.clone()
            return torch.dot(u, torch.mv(wm, v)).reshape(1)

    def forward(self, x):
        return F.conv1d(x, self.weight_orig / self.sigma(), self.bias, padding=self.padding)


class PlainConv1d(nn.Conv1d):
    """use_specnorm=False: nn.Conv1d (keys weight, bias) with the interface the head route reads."""

    @property
    def weight_orig(self):
        return self.weight

    def sigma(self):
        return torch.ones(1, dtype=torch.float32, device=self.weight.device)


class BatchNormLocal(nn.Module):
    """models/dinodisc.py:29-56: batch statistics over virtual groups of `virtual_bs` samples -- G = ceil(B / virtual_bs) groups of B / G samples (a B that does
    not split evenly raises, as the reference's `view` does), per (group, channel) over samples x tokens, biased variance, f32, eps inside the sqrt; the same in
    eval mode.  x: [B, C, L]."""

    def __init__(self, num_features, virtual_bs=8, eps=1e-6):
        super().__init__()
        self.virtual_bs, self.eps = virtual_bs, eps
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))

    def groups_for(self, b: int) -> int:
        g = int(np.ceil(b / self.virtual_bs))
        if b % g != 0:
            raise RuntimeError(f"BatchNormLocal: a batch of {b} does not split into {g} equal virtual groups (models/dinodisc.py:45-46)")
        return g

    def forward(self, x):
        shape = x.shape
        x = x.float().reshape(self.groups_for(shape[0]), -1, shape[-2], shape[-1])
        mean = x.mean([1, 3], keepdim=True)
        var = x.var([1, 3], keepdim=True, unbiased=False)
        x = (x - mean) / torch.sqrt(var + self.eps)
        return (x * self.weight[None, :, None] + self.bias[None, :, None]).reshape(shape)


class ResidualBlock(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn
        self.ratio = 1 / np.sqrt(2)

    def forward(self, x):
        return (self.fn(x) + x) * self.ratio


def make_block(channels, kernel_size, norm_type, norm_eps, use_specnorm):
    if norm_type == "bn":
        norm = BatchNormLocal(channels, eps=norm_eps)
    elif norm_type == "gn":
        norm = nn.GroupNorm(32, channels, eps=norm_eps, affine=True)
    elif norm_type in ("sbn", "lbn", "hbn"):
        if not _SYNCBN_HEADS:
            raise NotImplementedError(f"norm_type {norm_type!r}: the SyncBatchNorm head variants of models/dinodisc.py:62-65 are behind a switch that is off; "
                                      "dmvae_amd.models.dinodisc.enable_syncbn_heads() turns it on (run_on_mi355x.py --hip-dinodisc does)")
        from .. import dist
        norm = nn.SyncBatchNorm(channels, eps=norm_eps, process_group=None if norm_type == "sbn" else dist.new_local_machine_group())
    else:
        raise NotImplementedError
    conv = (SpectralConv1d if use_specnorm else PlainConv1d)(channels, channels, kernel_size, padding=kernel_size // 2)
    if not use_specnorm:
        nn.init.zeros_(conv.bias)
    return nn.Sequential(conv, norm, nn.LeakyReLU(0.2))


class DinoDisc(nn.Module):
    def __init__(self, ks, device, dino_ckpt, norm_type="bn", norm_eps=1e-6, use_specnorm=True, dino_size="vit_small", key_depths=(2, 5, 8, 11), *,
                 dino_depth=None):
        super().__init__()
        if dino_size not in _ARCH:
            raise ValueError(f"dino_size {dino_size!r}; known: {sorted(_ARCH)}")
        cfg = dict(_ARCH[dino_size])
        if dino_depth is not None:
            cfg["depth"] = int(dino_depth)            # reduced backbones for tests
        dino = DinoBackbone(**cfg)
        if dino_ckpt is None:
            warnings.warn("DinoDisc: no DINOv2 checkpoint given; the backbone is randomly initialised", stacklevel=2)
        else:
            dino.load_state_dict(torch.load(dino_ckpt, weights_only=True), strict=True)
        self.dino = [dino.to(device=device)]          # in a list: outside parameters() and the state_dict, as in the reference
        self.dino[0].requires_grad_(False)
        self.dino[0].eval()
        mean, std = torch.tensor((0.485, 0.456, 0.406)), torch.tensor((0.229, 0.224, 0.225))
        self.register_buffer("x_scale", (0.5 / std).reshape(1, 3, 1, 1))
        self.register_buffer("x_shift", ((0.5 - mean) / std).reshape(1, 3, 1, 1))
        self.key_depths = tuple(key_depths)
        self.norm_type = norm_type
        c = dino.embed_dim
        conv = SpectralConv1d if use_specnorm else PlainConv1d
        self.heads = nn.ModuleList([
            nn.Sequential(make_block(c, 1, norm_type, norm_eps, use_specnorm),
                          ResidualBlock(make_block(c, ks, norm_type, norm_eps, use_specnorm)),
                          conv(c, 1, 1, padding=0))
            for _ in self.key_depths])
        if not use_specnorm:
            for h in self.heads:
                nn.init.zeros_(h[2].bias)

    # ---- the backbone follows the module's device, and nothing else --------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        super()._apply(fn, *a, **k)
        if self.x_scale.device != self.dino[0].pos_embed.device:         # .to(device) / .cuda() / .cpu(): the frozen backbone moves along (dtype casts do not touch it)
            self.dino[0].to(self.x_scale.device)
        return self

    def preprocess(self, x: torch.Tensor) -> torch.Tensor:
        """models/dinodisc.py:166-178, f32 with autocast off: ImageNet normalisation of a [-1, 1] image, then a size that is a multiple of the patch: a random
        crop or an area resize (one `random.random()` decides) when both sides exceed it, else a bicubic resize."""
        with torch.autocast(x.device.type, enabled=False):
            x = self.x_scale * x.float() + self.x_shift
            h, w = x.shape[-2:]
            p = self.dino[0].patch_size
            nh, nw = h // p * p, w // p * p
            if h > nh and w > nw:
                if random.random() <= 0.5:
                    i = int(torch.randint(0, h - nh + 1, size=(1,)).item())
                    j = int(torch.randint(0, w - nw + 1, size=(1,)).item())
                    x = x[..., i:i + nh, j:j + nw]
                else:
                    x = F.interpolate(x, size=(nh, nw), mode="area")
            else:
                x = F.interpolate(x, size=(nh, nw), mode="bicubic")
        return x.contiguous()

    def _hip_route(self, x: torch.Tensor):
        """None when the HIP route takes this call, else why not."""
        from .. import parity
        from .vit_fast import hip_path_supported
        if not x.is_cuda:
            return "CPU tensor"
        if parity.on():
            return "the fp32 parity mode is not built for DinoDisc"
        if not (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16):
            return "outside autocast(bfloat16) (the HIP route implements the reference's autocast arithmetic)"
        vit = self.dino[0]
        if not hip_path_supported(vit, 0) or vit.embed_dim % 128 != 0 or vit.embed_dim > 512:
            return (f"backbone width {vit.embed_dim} with {vit.blocks[0].attn.num_heads} heads is outside the kernels' range (the heads' norm kernels take up to 512 "
                    "channels: ViT-S, the scripts' backbone)")
        return None

    def forward(self, x, grad_ckpt=False):       # x: image in [-1, 1]
        why = self._hip_route(x)
        if why is not None:
            from .._stock import require_opt_in
            require_opt_in("DinoDisc.forward", why)
            return self.forward_stock(x, grad_ckpt)
        from functools import partial
        from ..functional import DinoHeadEvalFn, DinoHeadFn
        from .patchgan import _bn_stats
        from .vit_fast import frozen_forward_features, frozen_taps_with_input_grad
        vit = self.dino[0]
        x = self.preprocess(x)
        b = x.shape[0]
        pos = vit.pos_for(x.shape[-2], x.shape[-1])
        if torch.is_grad_enabled() and x.requires_grad:
            taps = frozen_taps_with_input_grad(vit, x, self.key_depths, pos)
        else:
            taps = frozen_forward_features(vit, x, self.key_depths, pos)
        out = []
        for head, t in zip(self.heads, taps):
            c0, n0 = head[0][0], head[0][1]
            c1, n1 = head[1].fn[0], head[1].fn[1]
            c2 = head[2]
            if isinstance(n0, nn.SyncBatchNorm):
                if not (n0.training or not n0.track_running_stats) and not (torch.is_grad_enabled() and any(p.requires_grad for p in head.parameters())):
                    bn0, bn1 = ((n.running_mean, n.running_var, n.weight.detach(), n.bias.detach()) for n in (n0, n1))
                    out.append(DinoHeadEvalFn.apply(t, n0.eps, c0.weight_orig.detach(), c0.sigma().detach(), c0.bias.detach(), bn0, c1.weight_orig.detach(),
                                                    c1.sigma().detach(), c1.bias.detach(), bn1, c2.weight_orig.detach(), c2.sigma().detach(),
                                                    c2.bias.detach()).view(b, -1))
                    continue
                cfg = (1, t.shape[-1], n0.eps, (partial(_bn_stats, n0), partial(_bn_stats, n1)))
            elif self.norm_type == "bn":
                cfg = (n0.groups_for(b), t.shape[-1], n0.eps)
            else:
                cfg = (b, 32, n0.eps)
            out.append(DinoHeadFn.apply(t, cfg, c0.weight_orig, c0.sigma(), c0.bias, n0.weight, n0.bias, c1.weight_orig, c1.sigma(), c1.bias, n1.weight, n1.bias,
                                        c2.weight_orig, c2.sigma(), c2.bias).view(b, -1))
        return torch.cat(out, dim=1)

    def forward_stock(self, x, grad_ckpt=False):
        """The module in plain PyTorch (ATen / library kernels under autocast on a GPU; the definition on the CPU)."""
        x = self.preprocess(x)
        b = x.shape[0]
        out = []
        for head, t in zip(self.heads, self.dino[0].taps_stock(x, self.key_depths)):
            act = (t[:, 1:].float() + t[:, :1].float()).transpose(1, 2)
            if grad_ckpt:
                out.append(torch.utils.checkpoint.checkpoint(head, act, use_reentrant=False).view(b, -1))
            else:
                out.append(head(act).view(b, -1))
        return torch.cat(out, dim=1)
