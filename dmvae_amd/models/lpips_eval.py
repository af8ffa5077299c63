"""The evaluation LPIPS' three networks on the exact-f32 convolution / pool kernels of csrc/inception.hip and the f64 head of csrc/lpips_eval.hip: what they
share (`LPIPSEval`), and the `net_type='vgg'` and `'squeeze'` networks (`LPIPSVGG`, `LPIPSSqueeze`).  `net_type='alex'` is dmvae_amd/models/lpips_alex.py.

evaluation/metrics.py:26-29 is `LPIPS(img1, img2, net_type='alex')` and hands `net_type` to torchmetrics' `LearnedPerceptualImagePatchSimilarity`, which
takes 'alex', 'vgg' and 'squeeze': the LPIPS v0.1 variants.  All three are one scheme -- s = (x - shift) / scale per channel (f32);  a torchvision `features`
trunk tapped after chosen ReLUs;  per tap and pixel n = f / sqrt(eps + sum_c f_c^2);  d_l = mean_{h,w} sum_c lin_l[c] (n1_c - n2_c)^2;  per image
v = sum_l d_l -- and differ in the trunk, the taps and the number of `lin` heads.  `forward` returns v as f64 [N]; the library's `reduction='mean'` is
`forward(...).mean()` (dmvae_amd.metrics.LPIPS).

`LPIPSVGG`: torchvision's `vgg16.features`, the table of the reference's own utils/lpips.py:116-153 -- convolutions at indices 0, 2, 5, 7, 10, 12, 14, 17,
19, 21, 24, 26, 28, all 3 x 3 padding 1 with a ReLU, a 2 x 2 stride-2 max pool in front of slices 2 .. 5, taps after relu1_2, relu2_2, relu3_3, relu4_3,
relu5_3 (64, 128, 256, 512, 512 channels).  Names: `net.slice{1..5}.{idx}.weight|bias`, `lin{0..4}.model.1.weight`: the file `--lpips_path` hands the
tokenizer trainer plus torchvision's trunk.  `normalize="reference"` selects the reference's own normalisation n = f / (sqrt(sum_c f_c^2) + 1e-10)
(utils/lpips.py:156-158): the exact-f32 / f64 twin of the bf16 training loss `dmvae_amd.utils.lpips.LPIPS`, whose return value is `forward(...).mean()`;
`from_training(module)` copies that module's parameters.

`LPIPSSqueeze`: torchvision's `squeezenet1_1.features` as the LPIPS package slices it -- slice 1 [0, 1]: conv 3 -> 64 3 x 3 stride 2 no padding, ReLU;
slice 2 [2, 3, 4]: max pool 3 x 3 stride 2 ceil_mode, Fire(64; 16, 64, 64), Fire(128; 16, 64, 64);  slice 3 [5, 6, 7]: pool, Fire(128; 32, 128, 128),
Fire(256; 32, 128, 128);  slice 4 [8, 9]: pool, Fire(256; 48, 192, 192);  slice 5 [10]: Fire(384; 48, 192, 192);  slice 6 [11]: Fire(384; 64, 256, 256);
slice 7 [12]: Fire(512; 64, 256, 256).  A Fire module is squeeze 1 x 1 + ReLU, then the concatenation of expand 1 x 1 + ReLU and expand 3 x 3 padding 1 +
ReLU: the two expands write their halves of one NHWC buffer, there is no concat kernel.  Seven taps (64, 128, 256, 384, 384, 512, 512 channels), `lin0` ..
`lin6`.  Names: `net.slice1.0.weight|bias`, `net.slice{i}.{idx}.squeeze|expand1x1|expand3x3.weight|bias`.  THIS TABLE IS WRITTEN FROM MEMORY OF THE
PUBLISHED DEFINITION: neither torchvision, torchmetrics nor the `lpips` package is on any machine this package is developed on.

What is NOT here: the weight files (they are on no machine this package is developed on), and a run against torchmetrics itself: the library cannot be
run there either, so the networks are restated from their published definitions and tested, with seeded random parameters, against an independent f64
restatement (tests/lpips_eval_nets_spec.py).  A fresh module holds NaN in every parameter -- nothing is ever silently random -- until `load_state_dict`,
`from_checkpoint`, `from_checkpoints` or `from_training`; a conv or lin tensor missing from a file is a KeyError naming it.  On load the aliases
`lins.{k}.model.1.weight` (the published module registers its heads twice) and a torchvision-layout trunk (`features.N.*`; `classifier.*` is ignored) are
accepted too.

The arithmetic: both branches run through the trunk as ONE batch of 2 N images (`ops.lpips_input` writes them NHWC f32, scaled), every convolution is
`ops.conv2d_f32` (one k-ordered f32 fma chain per output, the bias as the epilogue's shift, the ReLU in the epilogue), the pools `ops.pool2d_f32` /
`ops.maxpool2d_f32`, and after each tap `ops.lpips_head` widens the features to f64 and forms the level's value with fixed-order sums, adding it to the
running v.  An image pair's value does not depend on its batch, its position in it or `chunk`, repeats bit for bit, `forward(x, x)` is exactly 0 and
`forward(a, b)` equals `forward(b, a)` bit for bit.  Measured on an MI355X: DESIGN.md 3.9, tools/bench_lpips_eval.py.

The operand packs are built on the first call and again whenever a parameter's `_version` or storage moves (`load_state_dict`, `.to()`, in-place ops under
`no_grad`); a write through `.data` moves no `_version`: call `refresh()` after one.  Inference only, all parameters frozen.  CPU tensors take the stock f32
composition (`forward_stock`) behind `DMVAE_ALLOW_STOCK=1`, like every other module (dmvae_amd/_stock.py)."""
from __future__ import annotations

import re
from typing import Dict, Iterator, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _stock, ops

__all__ = ["LPIPSEval", "LPIPSVGG", "LPIPSSqueeze", "SHIFT", "SCALE", "VGG_TRUNK", "SQUEEZE_TRUNK", "NORMALIZE"]

SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
NORMALIZE = {"torchmetrics": 0, "reference": 1}      # -> the head's form (include/dmvae_hip.h: dmvae_lpips_head_form)


def _nan_(m: nn.Module) -> nn.Module:
    for p in m.parameters():
        p.requires_grad_(False)
        p.fill_(float("nan"))
    return m


class LPIPSEval(nn.Module):
    """What the three networks share: the scaling-layer constants and their check on load, NaN-filled fresh parameters, the operand packs keyed on
    `_version`, the input checks, chunking, `forward`, `taps`, `forward_stock` and the CPU opt-in.  A subclass sets `min_size`, `_min_size_why`, `channels`,
    `_FEATURE_SLICE` / `_FEATURE_TAIL` (torchvision's `features.N.<tail>` -> `net.<slice>.N.<tail>`) and implements `_build_trunk` (fills `self.net`),
    `convs` (the trunk's convolutions in pack order), `_hip_taps` and `_stock_taps`."""

    min_size: int = 1
    _min_size_why: str = ""
    channels: Tuple[int, ...] = ()
    _FEATURE_SLICE: Dict[int, str] = {}
    _FEATURE_TAIL = r"(weight|bias)"
    head_form = 0

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
        self._build_trunk()
        for level, c in enumerate(self.channels):
            lin = nn.Module()
            lin.model = nn.Module()
            lin.model.add_module("1", _nan_(nn.Conv2d(c, 1, 1, bias=False)))
            self.add_module(f"lin{level}", lin)
        self._packs: Optional[dict] = None
        self._packs_key = None
        self.eval()

    # ---- what a subclass supplies ---------------------------------------------------------------------
    def _build_trunk(self) -> None:
        raise NotImplementedError

    def convs(self) -> List[nn.Conv2d]:
        raise NotImplementedError

    def _hip_taps(self, a: torch.Tensor, b: torch.Tensor, packs: dict, each) -> None:
        """Runs the trunk on one chunk (both halves as one batch) and calls each(level, tap NHWC f32 [2 n, h, w, c]) after every tapped ReLU."""
        raise NotImplementedError

    def _stock_taps(self, x: torch.Tensor) -> Iterator[torch.Tensor]:
        """x: the scaled NCHW f32 batch -> the tapped feature maps, through F.conv2d / F.max_pool2d."""
        raise NotImplementedError

    # ---- parameters in --------------------------------------------------------------------------------
    def lins(self) -> List[nn.Conv2d]:
        return [getattr(getattr(self, f"lin{k}").model, "1") for k in range(len(self.channels))]

    @classmethod
    def canonical_state_dict(cls, state_dict) -> Dict[str, torch.Tensor]:
        """The published names from any accepted layout: `lins.k.` -> `lin{k}.`, `features.N.` -> `net.slice{i}.N.`, `classifier.*` dropped."""
        out = {}
        for k, v in state_dict.items():
            m = re.match(r"lins\.(\d)\.(.*)$", k)
            if m:
                out.setdefault(f"lin{m.group(1)}.{m.group(2)}", v)
                continue
            m = re.match(rf"features\.(\d+)\.{cls._FEATURE_TAIL}$", k)
            if m and int(m.group(1)) in cls._FEATURE_SLICE:
                out[f"net.{cls._FEATURE_SLICE[int(m.group(1))]}.{k.split('.', 1)[1]}"] = v
                continue
            if k.startswith("classifier.") or k.startswith("features."):
                continue
            out[k] = v
        return out

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        name = type(self).__name__
        sd = self.canonical_state_dict(state_dict)
        own = self.state_dict()
        for k in own:
            if k.startswith("scaling_layer."):
                if k in sd and not torch.equal(sd[k].detach().float().cpu().reshape(-1), own[k].float().cpu().reshape(-1)):
                    raise ValueError(f"{name}: {k} = {sd[k].flatten().tolist()} is not the published constant {own[k].flatten().tolist()} the input kernel holds")
                sd[k] = own[k]
            elif k not in sd:
                raise KeyError(f"{name}: the checkpoint holds no tensor for {k} (nor under its lins.* / features.* alias)")
        return super().load_state_dict(sd, strict, **kw)

    @classmethod
    def from_checkpoint(cls, path, **kw):
        """One state_dict file holding the trunk and the lin weights, in any of the accepted layouts."""
        net = cls(**kw)
        net.load_state_dict(torch.load(path, map_location="cpu"))
        return net

    @classmethod
    def from_checkpoints(cls, trunk_path, lin_path, **kw):
        """torchvision's state_dict of the trunk (`features.N.*`, `classifier.*`) and the LPIPS v0.1 lin file (`lin{k}.model.1.weight`)."""
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
            raise ValueError(f"{type(self).__name__}: input on {device}, parameters on {tensors[0].device}; move the module with .to(device)")
        packs = {"conv": [(ops.pack_conv_weight_f32(m.weight), m.bias.detach().contiguous()) for m in self.convs()],
                 "lin": [m.weight.detach().reshape(-1).contiguous() for m in self.lins()]}
        self._packs, self._packs_key = packs, key
        return packs

    # ---- the HIP route --------------------------------------------------------------------------------
    def _check(self, img1: torch.Tensor, img2: torch.Tensor, check_range: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        name = type(self).__name__
        if not (torch.is_tensor(img1) and torch.is_tensor(img2)) or img1.dim() != 4 or img1.shape[1] != 3 or img1.shape != img2.shape or img1.shape[0] == 0:
            raise ValueError(f"{name}: expected two non-empty [N, 3, H, W] tensors of one shape, got "
                             f"{tuple(getattr(img1, 'shape', ()))} and {tuple(getattr(img2, 'shape', ()))}")
        if img1.device != img2.device:
            raise ValueError(f"{name}: the two inputs are on {img1.device} and {img2.device}")
        if img1.shape[2] < self.min_size or img1.shape[3] < self.min_size:
            raise ValueError(f"{name}: the trunk needs images of at least {self.min_size} x {self.min_size} ({self._min_size_why}), "
                             f"got {img1.shape[2]} x {img1.shape[3]}")
        if img1.dtype != img2.dtype or img1.dtype not in (torch.float32, torch.bfloat16):
            img1, img2 = img1.float(), img2.float()
        if check_range:
            (lo1, hi1), (lo2, hi2) = torch.aminmax(img1), torch.aminmax(img2)
            lo, hi = torch.stack([torch.minimum(lo1, lo2), torch.maximum(hi1, hi2)]).float().tolist()      # NaN propagates; one copy to the host
            if not (lo >= -1.0 and hi <= 1.0):                          # NaN fails too
                raise ValueError(f"{name}: expected both inputs in [-1, 1] (the library's own check), got values in [{lo}, {hi}]")
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
            _stock.require_opt_in(f"{type(self).__name__}.forward", "CPU images")
            return self.forward_stock(img1.float(), img2.float()).double()
        img1, img2 = img1.contiguous(), img2.contiguous()
        packs = self._operands(img1.device)
        n, step = img1.shape[0], self._step(chunk)
        out = torch.empty(n, dtype=torch.float64, device=img1.device)
        for i in range(0, n, step):
            v = out[i:min(n, i + step)]
            self._hip_taps(img1[i:i + step], img2[i:i + step], packs,
                           lambda level, f: ops.lpips_head(f, packs["lin"][level], self.eps, out=v, accumulate=level > 0, form=self.head_form))
        return out

    @torch.no_grad()
    def taps(self, img1: torch.Tensor, img2: torch.Tensor, *, chunk: Optional[int] = None) -> List[torch.Tensor]:
        """The tapped feature maps of the HIP route, NHWC f32 [2 N, h, w, c] each: rows 0 .. N are img1's, rows N .. 2 N img2's (what the tests compare
        with the f64 specification)."""
        img1, img2 = self._check(img1, img2, True)
        img1, img2 = img1.contiguous(), img2.contiguous()
        packs = self._operands(img1.device)
        n, step = img1.shape[0], self._step(chunk)
        levels = len(self.channels)
        firsts, seconds = [[] for _ in range(levels)], [[] for _ in range(levels)]

        def keep(level, f):
            firsts[level].append(f[:f.shape[0] // 2])
            seconds[level].append(f[f.shape[0] // 2:])
        for i in range(0, n, step):
            self._hip_taps(img1[i:i + step], img2[i:i + step], packs, keep)
        return [torch.cat(firsts[k] + seconds[k]) for k in range(levels)]

    # ---- the stock f32 composition -------------------------------------------------------------------
    @torch.no_grad()
    def forward_stock(self, img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
        """f32 [N, 3, H, W] pairs -> f32 [N] through F.conv2d / F.max_pool2d and the library's own f32 head arithmetic, on the tensors' device."""
        shift, scale = self.scaling_layer.shift, self.scaling_layer.scale
        x = torch.cat([(img1 - shift) / scale, (img2 - shift) / scale])
        n = img1.shape[0]
        total = None
        for x, lin in zip(self._stock_taps(x), self.lins()):
            if self.head_form == 0:
                nrm = x / torch.sqrt(self.eps + torch.sum(x ** 2, dim=1, keepdim=True))
            else:
                nrm = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + self.eps)
            d = F.conv2d((nrm[:n] - nrm[n:]) ** 2, lin.weight).mean(dim=(2, 3)).view(n)
            total = d if total is None else total + d
        return total


# ---- net_type 'vgg' ----------------------------------------------------------------------------------------------------------------------------
# (slice, index in torchvision's vgg16.features, cin, cout, a 2 x 2 stride-2 max pool in front, tapped after its ReLU): utils/lpips.py:116-153
VGG_TRUNK = (("slice1", 0, 3, 64, False, False), ("slice1", 2, 64, 64, False, True),
             ("slice2", 5, 64, 128, True, False), ("slice2", 7, 128, 128, False, True),
             ("slice3", 10, 128, 256, True, False), ("slice3", 12, 256, 256, False, False), ("slice3", 14, 256, 256, False, True),
             ("slice4", 17, 256, 512, True, False), ("slice4", 19, 512, 512, False, False), ("slice4", 21, 512, 512, False, True),
             ("slice5", 24, 512, 512, True, False), ("slice5", 26, 512, 512, False, False), ("slice5", 28, 512, 512, False, True))


class LPIPSVGG(LPIPSEval):
    """Two [N, 3, H, W] image batches in [-1, 1] (f32 or bf16, H, W >= 16) -> per-image LPIPS values f64 [N], net_type 'vgg'.  normalize: "torchmetrics"
    (n = f / sqrt(eps + sum f^2), eps 1e-8: the library's) or "reference" (n = f / (sqrt(sum f^2) + eps), eps 1e-10: utils/lpips.py:156-158, the training
    loss's own).  eps: None takes the normalisation's default.  chunk: image pairs per pass of the network."""

    min_size, _min_size_why = 16, "its four 2 x 2 pools leave relu5_3 a 1 x 1 map at that size"
    channels = tuple(t[3] for t in VGG_TRUNK if t[5])
    _FEATURE_SLICE = {idx: name for name, idx, *_ in VGG_TRUNK}

    def __init__(self, eps: Optional[float] = None, chunk: int = 16, normalize: str = "torchmetrics"):
        if normalize not in NORMALIZE:
            raise ValueError(f"normalize: expected one of {sorted(NORMALIZE)}, got {normalize!r}")
        super().__init__((1e-8, 1e-10)[NORMALIZE[normalize]] if eps is None else eps, chunk)
        self.normalize, self.head_form = normalize, NORMALIZE[normalize]

    def _build_trunk(self) -> None:
        for name, idx, cin, cout, _, _ in VGG_TRUNK:
            if not hasattr(self.net, name):
                self.net.add_module(name, nn.Module())
            getattr(self.net, name).add_module(str(idx), _nan_(nn.Conv2d(cin, cout, 3, 1, 1)))

    def convs(self) -> List[nn.Conv2d]:
        return [getattr(getattr(self.net, name), str(idx)) for name, idx, *_ in VGG_TRUNK]

    @classmethod
    def from_training(cls, module, **kw) -> "LPIPSVGG":
        """A `dmvae_amd.utils.lpips.LPIPS` (the bf16 training loss) with its trunk loaded -> this network holding copies of its parameters.  With
        normalize="reference" the result's `forward(a, b).mean()` is the exact-f32 / f64 value of what that module's forward computes in bf16."""
        if not getattr(module, "trunk_loaded", False):
            raise ValueError("LPIPSVGG.from_training: the module's VGG16 trunk holds no loaded weights (LPIPS.load_trunk)")
        sd = {}
        for name, idx, *_ in VGG_TRUNK:
            conv = getattr(getattr(module.net, name), str(idx))
            sd[f"net.{name}.{idx}.weight"], sd[f"net.{name}.{idx}.bias"] = conv.weight.detach().float().clone(), conv.bias.detach().float().clone()
        for k in range(5):
            sd[f"lin{k}.model.1.weight"] = getattr(module, f"lin{k}").model[-1].weight.detach().float().clone()
        sd["scaling_layer.shift"], sd["scaling_layer.scale"] = module.scaling_layer.shift.detach(), module.scaling_layer.scale.detach()
        net = cls(**kw)
        net.load_state_dict(sd)
        return net.to(module.lin0.model[-1].weight.device)

    def _hip_taps(self, a, b, packs, each) -> None:
        x, level = ops.lpips_input(a, b), 0
        for (_, _, _, _, pool, tap), (w, bias) in zip(VGG_TRUNK, packs["conv"]):
            if pool:
                x = ops.maxpool2d_f32(x, 2, 2)
            x = ops.conv2d_f32(x, w, (3, 3), 1, (1, 1), None, bias, True)
            if tap:
                each(level, x)
                level += 1

    def _stock_taps(self, x):
        for (_, _, _, _, pool, tap), conv in zip(VGG_TRUNK, self.convs()):
            if pool:
                x = F.max_pool2d(x, 2, 2)
            x = F.relu(F.conv2d(x, conv.weight, conv.bias, 1, 1))
            if tap:
                yield x


# ---- net_type 'squeeze' ------------------------------------------------------------------------------------------------------------------------
# (slice, index in torchvision's squeezenet1_1.features, cin, squeeze, expand 1 x 1, expand 3 x 3, a 3 x 3 stride-2 ceil_mode max pool in front): the Fire
# modules; every one is the last layer of its slice or is followed by another Fire of the same slice -- `tap` marks the slice's end.  features[0], the
# 3 -> 64 3 x 3 stride 2 convolution of slice 1, is tap 0.
SQUEEZE_STEM = ("slice1", 0, 3, 64)
SQUEEZE_TRUNK = (("slice2", 3, 64, 16, 64, 64, True, False), ("slice2", 4, 128, 16, 64, 64, False, True),
                 ("slice3", 6, 128, 32, 128, 128, True, False), ("slice3", 7, 256, 32, 128, 128, False, True),
                 ("slice4", 9, 256, 48, 192, 192, True, True), ("slice5", 10, 384, 48, 192, 192, False, True),
                 ("slice6", 11, 384, 64, 256, 256, False, True), ("slice7", 12, 512, 64, 256, 256, False, True))


def _squeeze_min_size() -> int:
    """The smallest side at which each of the three pools still sees at least 3 rows (a 3 x 3 window no smaller than the map it is laid on)."""
    size = 3
    while True:
        h, ok = (size - 3) // 2 + 1, True
        for *_, pool, _ in SQUEEZE_TRUNK:
            if pool:
                ok, h = ok and h >= 3, (h - 2) // 2 + 1
        if ok:
            return size
        size += 1


class LPIPSSqueeze(LPIPSEval):
    """Two [N, 3, H, W] image batches in [-1, 1] (f32 or bf16, H, W >= 25) -> per-image LPIPS values f64 [N], net_type 'squeeze' (SqueezeNet 1.1, seven
    taps).  The layer table is written from memory of the published definition (module docstring)."""

    min_size, _min_size_why = _squeeze_min_size(), "its third 3 x 3 pool is given a 3 x 3 map at that size"
    channels = (SQUEEZE_STEM[3],) + tuple(t[4] + t[5] for t in SQUEEZE_TRUNK if t[7])
    _FEATURE_SLICE = {SQUEEZE_STEM[1]: SQUEEZE_STEM[0], **{idx: name for name, idx, *_ in SQUEEZE_TRUNK}}
    _FEATURE_TAIL = r"(?:(?:squeeze|expand1x1|expand3x3)\.)?(weight|bias)"

    def __init__(self, eps: float = 1e-8, chunk: int = 64):
        super().__init__(eps, chunk)

    def _build_trunk(self) -> None:
        name, idx, cin, cout = SQUEEZE_STEM
        self.net.add_module(name, nn.Module())
        getattr(self.net, name).add_module(str(idx), _nan_(nn.Conv2d(cin, cout, 3, 2, 0)))
        for name, idx, cin, sq, e1, e3, _, _ in SQUEEZE_TRUNK:
            if not hasattr(self.net, name):
                self.net.add_module(name, nn.Module())
            fire = nn.Module()
            fire.squeeze, fire.expand1x1, fire.expand3x3 = _nan_(nn.Conv2d(cin, sq, 1)), _nan_(nn.Conv2d(sq, e1, 1)), _nan_(nn.Conv2d(sq, e3, 3, 1, 1))
            getattr(self.net, name).add_module(str(idx), fire)

    def fires(self) -> List[nn.Module]:
        return [getattr(getattr(self.net, name), str(idx)) for name, idx, *_ in SQUEEZE_TRUNK]

    def convs(self) -> List[nn.Conv2d]:
        """features[0], then every Fire's squeeze, expand1x1, expand3x3."""
        out = [getattr(getattr(self.net, SQUEEZE_STEM[0]), str(SQUEEZE_STEM[1]))]
        for f in self.fires():
            out += [f.squeeze, f.expand1x1, f.expand3x3]
        return out

    def _hip_taps(self, a, b, packs, each) -> None:
        conv = packs["conv"]
        x = ops.conv2d_f32(ops.lpips_input(a, b), conv[0][0], (3, 3), 2, (0, 0), None, conv[0][1], True)
        each(0, x)
        level = 1
        for k, (_, _, _, _, e1, e3, pool, tap) in enumerate(SQUEEZE_TRUNK):
            if pool:
                x = ops.maxpool2d_f32(x, 3, 2, True)
            (wq, bq), (w1, b1), (w3, b3) = conv[1 + 3 * k:4 + 3 * k]
            s = ops.conv2d_f32(x, wq, (1, 1), 1, (0, 0), None, bq, True)
            x = torch.empty(*s.shape[:3], e1 + e3, dtype=torch.float32, device=s.device)      # the concat: each expand writes its channel slice
            ops.conv2d_f32(s, w1, (1, 1), 1, (0, 0), None, b1, True, out=x, c_offset=0)
            ops.conv2d_f32(s, w3, (3, 3), 1, (1, 1), None, b3, True, out=x, c_offset=e1)
            if tap:
                each(level, x)
                level += 1

    def _stock_taps(self, x):
        stem = self.convs()[0]
        x = F.relu(F.conv2d(x, stem.weight, stem.bias, 2, 0))
        yield x
        for (*_, pool, tap), f in zip(SQUEEZE_TRUNK, self.fires()):
            if pool:
                x = F.max_pool2d(x, 3, 2, ceil_mode=True)
            s = F.relu(F.conv2d(x, f.squeeze.weight, f.squeeze.bias))
            x = torch.cat([F.relu(F.conv2d(s, f.expand1x1.weight, f.expand1x1.bias)), F.relu(F.conv2d(s, f.expand3x3.weight, f.expand3x3.bias, 1, 1))], 1)
            if tap:
                yield x
