"""The evaluation LPIPS (AlexNet) on the exact-f32 convolution / pool kernels of csrc/inception.hip and the f64 head of csrc/lpips_eval.hip.

`LPIPSAlex` is the network behind evaluation/metrics.py:26-29: torchmetrics' `LearnedPerceptualImagePatchSimilarity(net_type='alex')`, i.e. the LPIPS
v0.1 AlexNet variant.  Its parameters and buffers carry the published module's names -- `net.slice1.0`, `net.slice2.3`, `net.slice3.6`, `net.slice4.8`,
`net.slice5.10` (`weight`, `bias`: torchvision's AlexNet `features` indices), `lin{0..4}.model.1.weight` [1, C, 1, 1] (no bias; the dropout in front is the
identity in eval mode) and the buffers `scaling_layer.shift` / `scaling_layer.scale` -- so `load_state_dict` takes the published file.  On load the aliases
`lins.{k}.model.1.weight` (the published module registers its heads twice) and a torchvision-layout trunk (`features.N.*`; `classifier.*` is ignored) are
accepted too.  This is NOT `dmvae_amd.utils.lpips` / utils/lpips.py: that is the training loss, VGG16 in bf16 with a backward, a different network with
different numbers.

What is NOT here: the weight files (they are on no machine this package is developed on), and a run against torchmetrics itself: the library cannot be
run there either, so the network is restated from its published definition and tested, with seeded random parameters, against an independent f64
restatement (tests/lpips_eval_spec.py).  A fresh module holds NaN in every parameter -- nothing is ever silently random -- until `load_state_dict`,
`from_checkpoint` or `from_checkpoints`; a conv or lin tensor missing from a file is a KeyError naming it.

What is computed, for two [N, 3, H, W] batches in [-1, 1]:  s = (x - shift) / scale per channel (f32);  AlexNet's `features` tapped after each of its five
ReLUs (conv 3->64 11x11 stride 4 pad 2, max pool 3x3 stride 2, conv 64->192 5x5 pad 2, max pool, conv 192->384, 384->256, 256->256 3x3 pad 1; all with
bias);  per tap and pixel n = f / sqrt(eps + sum_c f_c^2);  d_l = mean_{h,w} sum_c lin_l[c] (n1_c - n2_c)^2;  per image v = sum_l d_l.  `forward` returns
v as f64 [N]; the library's `reduction='mean'` is `forward(...).mean()` (dmvae_amd.metrics.LPIPS).

The arithmetic: both branches run through the trunk as ONE batch of 2 N images (`ops.lpips_input` writes them NHWC f32, scaled), every convolution is
`ops.conv2d_f32` (one k-ordered f32 fma chain per output, the bias as the epilogue's shift, the ReLU in the epilogue), the pools `ops.pool2d_f32`, and after
each tap `ops.lpips_head` widens the features to f64 and forms the level's value with fixed-order sums, adding it to the running v.  An image pair's value
does not depend on its batch, its position in it or `chunk`, repeats bit for bit, `forward(x, x)` is exactly 0 and `forward(a, b)` equals `forward(b, a)`
bit for bit.  Measured on an MI355X: DESIGN.md 3.9, tools/bench_lpips_eval.py.

The operand packs are built on the first call and again whenever a parameter's `_version` or storage moves (`load_state_dict`, `.to()`, in-place ops under
`no_grad`); a write through `.data` moves no `_version`: call `refresh()` after one.  Inference only, all parameters frozen.  CPU tensors take the stock f32
composition (`forward_stock`) behind `DMVAE_ALLOW_STOCK=1`, like every other module (dmvae_amd/_stock.py)."""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _stock, ops

__all__ = ["LPIPSAlex", "TRUNK", "SHIFT", "SCALE"]

SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
# (slice, index in torchvision's AlexNet.features, cin, cout, kernel, stride, padding, max pool in front)
TRUNK = (("slice1", 0, 3, 64, 11, 4, 2, False), ("slice2", 3, 64, 192, 5, 1, 2, True), ("slice3", 6, 192, 384, 3, 1, 1, True),
         ("slice4", 8, 384, 256, 3, 1, 1, False), ("slice5", 10, 256, 256, 3, 1, 1, False))
_FEATURE_SLICE = {idx: name for name, idx, *_ in TRUNK}


def _nan_(m: nn.Module) -> nn.Module:
    for p in m.parameters():
        p.requires_grad_(False)
        p.fill_(float("nan"))
    return m


class LPIPSAlex(nn.Module):
    """Two [N, 3, H, W] image batches in [-1, 1] (f32 or bf16, H, W >= 63) -> per-image LPIPS values f64 [N].  eps: the normalisation's epsilon (the
    library's constructor argument, default 1e-8; > 0).  chunk: image pairs per pass of the network."""

    min_size, channels = 63, tuple(t[3] for t in TRUNK)

    def __init__(self, eps: float = 1e-8, chunk: int = 64):
        super().__init__()
        if not (float(eps) > 0 and float(eps) != float("inf")):
            raise ValueError(f"eps: expected a finite positive number, got {eps}")
        if int(chunk) < 1:
            raise ValueError(f"chunk: expected >= 1, got {chunk}")
        self.eps, self.chunk = float(eps), int(chunk)
        self.scaling_layer = nn.Module()
        self.scaling_layer.register_buffer("shift", torch.tensor(SHIFT).view(1, 3, 1, 1))
        self.scaling_layer.register_buffer("scale", torch.tensor(SCALE).view(1, 3, 1, 1))
        self.net = nn.Module()
        for name, idx, cin, cout, k, stride, pad, _ in TRUNK:
            s = nn.Module()
            s.add_module(str(idx), _nan_(nn.Conv2d(cin, cout, k, stride, pad)))
            self.net.add_module(name, s)
        for level, c in enumerate(self.channels):
            lin = nn.Module()
            lin.model = nn.Module()
            lin.model.add_module("1", _nan_(nn.Conv2d(c, 1, 1, bias=False)))
            self.add_module(f"lin{level}", lin)
        self._packs: Optional[dict] = None
        self._packs_key = None
        self.eval()

    # ---- parameters in --------------------------------------------------------------------------------
    def convs(self) -> List[nn.Conv2d]:
        return [getattr(getattr(self.net, name), str(idx)) for name, idx, *_ in TRUNK]

    def lins(self) -> List[nn.Conv2d]:
        return [getattr(getattr(self, f"lin{k}").model, "1") for k in range(5)]

    @staticmethod
    def canonical_state_dict(state_dict) -> Dict[str, torch.Tensor]:
        """The published names from any accepted layout: `lins.k.` -> `lin{k}.`, `features.N.` -> `net.slice{i}.N.`, `classifier.*` dropped."""
        out = {}
        for k, v in state_dict.items():
            m = re.match(r"lins\.(\d)\.(.*)$", k)
            if m:
                out.setdefault(f"lin{m.group(1)}.{m.group(2)}", v)
                continue
            m = re.match(r"features\.(\d+)\.(weight|bias)$", k)
            if m and int(m.group(1)) in _FEATURE_SLICE:
                out[f"net.{_FEATURE_SLICE[int(m.group(1))]}.{m.group(1)}.{m.group(2)}"] = v
                continue
            if k.startswith("classifier.") or k.startswith("features."):
                continue
            out[k] = v
        return out

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        sd = self.canonical_state_dict(state_dict)
        own = self.state_dict()
        for k in own:
            if k.startswith("scaling_layer."):
                if k in sd and not torch.equal(sd[k].detach().float().cpu().reshape(-1), own[k].float().cpu().reshape(-1)):
                    raise ValueError(f"LPIPSAlex: {k} = {sd[k].flatten().tolist()} is not the published constant {own[k].flatten().tolist()} the input kernel holds")
                sd[k] = own[k]
            elif k not in sd:
                raise KeyError(f"LPIPSAlex: the checkpoint holds no tensor for {k} (nor under its lins.* / features.* alias)")
        return super().load_state_dict(sd, strict, **kw)

    @classmethod
    def from_checkpoint(cls, path, **kw) -> "LPIPSAlex":
        """One state_dict file holding the trunk and the five lin weights, in any of the accepted layouts."""
        net = cls(**kw)
        net.load_state_dict(torch.load(path, map_location="cpu"))
        return net

    @classmethod
    def from_checkpoints(cls, trunk_path, lin_path, **kw) -> "LPIPSAlex":
        """torchvision's AlexNet state_dict (`features.N.*`, `classifier.*`) and the LPIPS v0.1 `alex.pth` (`lin{k}.model.1.weight`)."""
        sd = dict(torch.load(trunk_path, map_location="cpu"))
        sd.update(torch.load(lin_path, map_location="cpu"))
        net = cls(**kw)
        net.load_state_dict(sd)
        return net

    def refresh(self) -> None:
        """Drops the operand packs: the next call rebuilds them (needed only after a write that moves no `_version`, e.g. through `.data`)."""
        self._packs = self._packs_key = None

    def _operands(self, device) -> dict:
        tensors = list(self.parameters())
        key = (str(device), tuple((t.data_ptr(), t._version) for t in tensors))
        if self._packs is not None and self._packs_key == key:
            return self._packs
        if any(t.device != device for t in tensors):
            raise ValueError(f"LPIPSAlex: input on {device}, parameters on {tensors[0].device}; move the module with .to(device)")
        packs = {"conv": [(ops.pack_conv_weight_f32(m.weight), m.bias.detach().contiguous()) for m in self.convs()],
                 "lin": [m.weight.detach().reshape(-1).contiguous() for m in self.lins()]}
        self._packs, self._packs_key = packs, key
        return packs

    # ---- the HIP route --------------------------------------------------------------------------------
    def _hip_taps(self, a: torch.Tensor, b: torch.Tensor, packs: dict, each) -> None:
        """Runs the trunk on one chunk (both halves as one batch) and calls each(level, tap NHWC f32 [2 n, h, w, c]) after every ReLU."""
        x = ops.lpips_input(a, b)
        for level, (_, _, _, _, k, stride, pad, pool) in enumerate(TRUNK):
            if pool:
                x = ops.pool2d_f32(x, ops.POOL_MAX_S2)
            w, bias = packs["conv"][level]
            x = ops.conv2d_f32(x, w, (k, k), stride, (pad, pad), None, bias, True)
            each(level, x)

    def _check(self, img1: torch.Tensor, img2: torch.Tensor, check_range: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        if not (torch.is_tensor(img1) and torch.is_tensor(img2)) or img1.dim() != 4 or img1.shape[1] != 3 or img1.shape != img2.shape or img1.shape[0] == 0:
            raise ValueError("LPIPSAlex: expected two non-empty [N, 3, H, W] tensors of one shape, got "
                             f"{tuple(getattr(img1, 'shape', ()))} and {tuple(getattr(img2, 'shape', ()))}")
        if img1.device != img2.device:
            raise ValueError(f"LPIPSAlex: the two inputs are on {img1.device} and {img2.device}")
        if img1.shape[2] < self.min_size or img1.shape[3] < self.min_size:
            raise ValueError(f"LPIPSAlex: the trunk needs images of at least {self.min_size} x {self.min_size} (its third convolution is given a 3 x 3 map "
                             f"at that size), got {img1.shape[2]} x {img1.shape[3]}")
        if img1.dtype != img2.dtype or img1.dtype not in (torch.float32, torch.bfloat16):
            img1, img2 = img1.float(), img2.float()
        if check_range:
            (lo1, hi1), (lo2, hi2) = torch.aminmax(img1), torch.aminmax(img2)
            lo, hi = torch.stack([torch.minimum(lo1, lo2), torch.maximum(hi1, hi2)]).float().tolist()      # NaN propagates; one copy to the host
            if not (lo >= -1.0 and hi <= 1.0):                          # NaN fails too
                raise ValueError(f"LPIPSAlex: expected both inputs in [-1, 1] (the library's own check), got values in [{lo}, {hi}]")
        return img1, img2

    def _step(self, chunk: Optional[int]) -> int:
        step = self.chunk if chunk is None else int(chunk)
        if step < 1:
            raise ValueError(f"chunk: expected >= 1, got {chunk}")
        return step

    @torch.no_grad()
    def forward(self, img1: torch.Tensor, img2: torch.Tensor, *, chunk: Optional[int] = None, check_range: bool = True) -> torch.Tensor:
        """-> f64 [N], the per-image values.  check_range=False skips the [-1, 1] check (one host synchronisation) for a caller that guarantees it."""
        img1, img2 = self._check(img1, img2, check_range)
        if not img1.is_cuda:
            _stock.require_opt_in("LPIPSAlex.forward", "CPU images")
            return self.forward_stock(img1.float(), img2.float()).double()
        img1, img2 = img1.contiguous(), img2.contiguous()
        packs = self._operands(img1.device)
        n, step = img1.shape[0], self._step(chunk)
        out = torch.empty(n, dtype=torch.float64, device=img1.device)
        for i in range(0, n, step):
            v = out[i:min(n, i + step)]
            self._hip_taps(img1[i:i + step], img2[i:i + step], packs,
                           lambda level, f: ops.lpips_head(f, packs["lin"][level], self.eps, out=v, accumulate=level > 0))
        return out

    @torch.no_grad()
    def taps(self, img1: torch.Tensor, img2: torch.Tensor, *, chunk: Optional[int] = None) -> List[torch.Tensor]:
        """The five tapped feature maps of the HIP route, NHWC f32 [2 N, h, w, c] each: rows 0 .. N are img1's, rows N .. 2 N img2's (what the tests compare
        with the f64 specification)."""
        img1, img2 = self._check(img1, img2, True)
        img1, img2 = img1.contiguous(), img2.contiguous()
        packs = self._operands(img1.device)
        n, step = img1.shape[0], self._step(chunk)
        firsts, seconds = [[] for _ in TRUNK], [[] for _ in TRUNK]

        def keep(level, f):
            firsts[level].append(f[:f.shape[0] // 2])
            seconds[level].append(f[f.shape[0] // 2:])
        for i in range(0, n, step):
            self._hip_taps(img1[i:i + step], img2[i:i + step], packs, keep)
        return [torch.cat(firsts[k] + seconds[k]) for k in range(len(TRUNK))]

    # ---- the stock f32 composition -------------------------------------------------------------------
    @torch.no_grad()
    def forward_stock(self, img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
        """f32 [N, 3, H, W] pairs -> f32 [N] through F.conv2d / F.max_pool2d and the library's own f32 head arithmetic, on the tensors' device."""
        shift, scale = self.scaling_layer.shift, self.scaling_layer.scale
        x = torch.cat([(img1 - shift) / scale, (img2 - shift) / scale])
        n = img1.shape[0]
        total = None
        for (_, _, _, _, _, stride, pad, pool), conv, lin in zip(TRUNK, self.convs(), self.lins()):
            if pool:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, conv.weight, conv.bias, stride, pad))
            nrm = x / torch.sqrt(self.eps + torch.sum(x ** 2, dim=1, keepdim=True))
            d = F.conv2d((nrm[:n] - nrm[n:]) ** 2, lin.weight).mean(dim=(2, 3)).view(n)
            total = d if total is None else total + d
        return total
