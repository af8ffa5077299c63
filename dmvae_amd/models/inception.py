"""The FID Inception-v3 feature extractor on the exact-f32 HIP kernels of csrc/inception.hip.

`InceptionV3Compat` is the network both of the reference's evaluations run their images through: evaluation/fid.py:8-48 (torchmetrics' `NoTrainInceptionV3`)
and sample_50k.py:174-209 (torch-fidelity's `inception-v3-compat`), i.e. torch-fidelity's `FeatureExtractorInceptionV3` with the
`pt_inception-2015-12-05` weights.  Its parameters and buffers carry that module's names -- `<layer>.conv.weight` (OIHW, no bias),
`<layer>.bn.{weight,bias,running_mean,running_var}` (eps 1e-3), `fc.weight` [1008, 2048], `fc.bias` [1008] -- so `load_state_dict` takes the published file
(`num_batches_tracked` keys are tolerated and ignored).

What is NOT here: the weight file (it is on no machine this package is developed on; a fresh module holds torch's default initialisation and is of no
use for a metric until `from_checkpoint` / `load_state_dict`), and a run against torch-fidelity itself.  As with the package's other torch-fidelity
definitions (csrc/fidelity.hip, csrc/manifold.hip) the network is restated from its published form and tested, with seeded random parameters, against an f64
restatement (tests/inception_spec.py).

The arithmetic: torch-fidelity runs the network in f32, and FID is sensitive to it, so every convolution (the fc layer included: a 1 x 1 convolution at
H = W = 1) is `ops.conv2d_f32`: f32 operands, f32 accumulation on v_mfma_f32_16x16x4_f32, one k-ordered fma chain per output, eval-mode BatchNorm as an
epilogue `acc * scale + shift` with scale = gamma / sqrt(var + eps), shift = beta - mean * scale formed in f64 on the host and rounded once (the weights
keep the checkpoint's bits: nothing is folded into them), then the ReLU.  Activations are NHWC f32; every branch of a Mixed block writes its slice of the
block's concat directly.  An image's result does not depend on its batch or its position in it, and repeats bit for bit; batches above `chunk` images
are therefore processed in chunks with no effect on any value.  Measured on an MI355X (tools/bench_inception.py) the route is SLOWER
than `forward_stock` on the same device: 2338 against 4126 images/s at B = 200; what it gives is the fixed arithmetic, not time.

The operand packs and the scale / shift vectors are built on the first call and again whenever a parameter's or buffer's `_version` or storage moves
(`load_state_dict`, `.to()`, in-place ops under `no_grad`).  A write through `.data` does not move `_version` (torch gives `.data` its own counter): call
`refresh()` after one.  Inference only.  CPU tensors take the stock f32 composition behind `DMVAE_ALLOW_STOCK=1`, like every other module
(dmvae_amd/_stock.py); `forward_stock` stays callable directly."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _stock, ops

__all__ = ["InceptionV3Compat", "LAYER_TABLE", "fid_module"]

BN_EPS = 1e-3
_POOLS = {"avg": ops.POOL_AVG_S1P1, "max1": ops.POOL_MAX_S1P1, "max2": ops.POOL_MAX_S2}


class _BatchNormEval(nn.Module):
    """The four tensors of an eval-mode BatchNorm2d under torch's names (no num_batches_tracked)."""

    def __init__(self, c: int):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.ones(c), requires_grad=False), nn.Parameter(torch.zeros(c), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))


class _ConvWeight(nn.Module):
    def __init__(self, cin: int, cout: int, kh: int, kw: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, kh, kw), requires_grad=False)
        nn.init.kaiming_normal_(self.weight, nonlinearity="relu")


class BasicConv2d(nn.Module):
    """conv (no bias) -> BatchNorm (eval, eps 1e-3) -> ReLU."""

    def __init__(self, cin: int, cout: int, kernel, stride: int = 1, padding=0):
        super().__init__()
        self.kernel = (kernel, kernel) if isinstance(kernel, int) else tuple(kernel)
        self.padding = (padding, padding) if isinstance(padding, int) else tuple(padding)
        self.cin, self.cout, self.stride = cin, cout, stride
        self.conv, self.bn = _ConvWeight(cin, cout, *self.kernel), _BatchNormEval(cout)

    def out_hw(self, h: int, w: int) -> Tuple[int, int]:
        return (h + 2 * self.padding[0] - self.kernel[0]) // self.stride + 1, (w + 2 * self.padding[1] - self.kernel[1]) // self.stride + 1

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """The stock composition on NCHW tensors of the parameters' dtype."""
        y = F.conv2d(x, self.conv.weight, None, self.stride, self.padding)
        return F.relu(F.batch_norm(y, self.bn.running_mean, self.bn.running_var, self.bn.weight, self.bn.bias, False, 0.0, BN_EPS))


# A block is a list of branches, concatenated in order; a branch is a list of steps: a BasicConv2d, a pool tag, or -- as the last step -- a tuple of
# BasicConv2d that all read the previous step's output and are concatenated.
class _BlockA(nn.Module):
    def __init__(self, cin: int, pool_features: int):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, 1)
        self.branch5x5_1, self.branch5x5_2 = BasicConv2d(cin, 48, 1), BasicConv2d(48, 64, 5, padding=2)
        self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3 = BasicConv2d(cin, 64, 1), BasicConv2d(64, 96, 3, padding=1), BasicConv2d(96, 96, 3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, 1)

    def plan(self):
        return [[self.branch1x1], [self.branch5x5_1, self.branch5x5_2], [self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3],
                ["avg", self.branch_pool]]


class _BlockB(nn.Module):
    def __init__(self, cin: int):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, 3, stride=2)
        self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3 = BasicConv2d(cin, 64, 1), BasicConv2d(64, 96, 3, padding=1), BasicConv2d(96, 96, 3, stride=2)

    def plan(self):
        return [[self.branch3x3], [self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3], ["max2"]]


class _BlockC(nn.Module):
    def __init__(self, cin: int, c7: int):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, 1)
        self.branch7x7_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7_2 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, (7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, (1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, 1)

    def plan(self):
        return [[self.branch1x1], [self.branch7x7_1, self.branch7x7_2, self.branch7x7_3],
                [self.branch7x7dbl_1, self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5], ["avg", self.branch_pool]]


class _BlockD(nn.Module):
    def __init__(self, cin: int):
        super().__init__()
        self.branch3x3_1, self.branch3x3_2 = BasicConv2d(cin, 192, 1), BasicConv2d(192, 320, 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, 1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, 3, stride=2)

    def plan(self):
        return [[self.branch3x3_1, self.branch3x3_2], [self.branch7x7x3_1, self.branch7x7x3_2, self.branch7x7x3_3, self.branch7x7x3_4], ["max2"]]


class _BlockE(nn.Module):
    def __init__(self, cin: int, pool: str):
        super().__init__()
        self.pool = pool
        self.branch1x1 = BasicConv2d(cin, 320, 1)
        self.branch3x3_1 = BasicConv2d(cin, 384, 1)
        self.branch3x3_2a, self.branch3x3_2b = BasicConv2d(384, 384, (1, 3), padding=(0, 1)), BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch3x3dbl_1, self.branch3x3dbl_2 = BasicConv2d(cin, 448, 1), BasicConv2d(448, 384, 3, padding=1)
        self.branch3x3dbl_3a, self.branch3x3dbl_3b = BasicConv2d(384, 384, (1, 3), padding=(0, 1)), BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, 1)

    def plan(self):
        return [[self.branch1x1], [self.branch3x3_1, (self.branch3x3_2a, self.branch3x3_2b)],
                [self.branch3x3dbl_1, self.branch3x3dbl_2, (self.branch3x3dbl_3a, self.branch3x3dbl_3b)], [self.pool, self.branch_pool]]


# (stage, constructor): the network in forward order; "MaxPool_*" are the two stride-2 pools of the stem
LAYER_TABLE = (
    ("Conv2d_1a_3x3", lambda: BasicConv2d(3, 32, 3, stride=2)), ("Conv2d_2a_3x3", lambda: BasicConv2d(32, 32, 3)),
    ("Conv2d_2b_3x3", lambda: BasicConv2d(32, 64, 3, padding=1)), ("MaxPool_1", None),
    ("Conv2d_3b_1x1", lambda: BasicConv2d(64, 80, 1)), ("Conv2d_4a_3x3", lambda: BasicConv2d(80, 192, 3)), ("MaxPool_2", None),
    ("Mixed_5b", lambda: _BlockA(192, 32)), ("Mixed_5c", lambda: _BlockA(256, 64)), ("Mixed_5d", lambda: _BlockA(288, 64)),
    ("Mixed_6a", lambda: _BlockB(288)),
    ("Mixed_6b", lambda: _BlockC(768, 128)), ("Mixed_6c", lambda: _BlockC(768, 160)), ("Mixed_6d", lambda: _BlockC(768, 160)), ("Mixed_6e", lambda: _BlockC(768, 192)),
    ("Mixed_7a", lambda: _BlockD(768)), ("Mixed_7b", lambda: _BlockE(1280, "avg")), ("Mixed_7c", lambda: _BlockE(2048, "max1")),
)


def _stock_step(step, x: torch.Tensor) -> torch.Tensor:
    if isinstance(step, str):
        if step == "avg":
            return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)
        return F.max_pool2d(x, 3, 1, 1) if step == "max1" else F.max_pool2d(x, 3, 2)
    if isinstance(step, tuple):
        return torch.cat([s(x) for s in step], 1)
    return step(x)


def _stock_block(block, x: torch.Tensor) -> torch.Tensor:
    outs = []
    for branch in block.plan():
        y = x
        for step in branch:
            y = _stock_step(step, y)
        outs.append(y)
    return torch.cat(outs, 1)


class InceptionV3Compat(nn.Module):
    """uint8 images -> 2048 pool features (`forward`, what `fid.FID(feature=net)` calls), or normalised f32 images -> (features, logits_unbiased)
    (`features_logits`, the `fidelity.FidelityMetrics` extractor contract; `extractor()` returns it).  chunk: images per pass of the network."""

    num_features, num_classes, input_size, min_size = 2048, 1008, 299, 75

    def __init__(self, chunk: int = 50):
        super().__init__()
        if int(chunk) < 1:
            raise ValueError(f"chunk: expected >= 1, got {chunk}")
        self.chunk = int(chunk)
        for name, make in LAYER_TABLE:
            if make is not None:
                self.add_module(name, make())
        self.fc = nn.Linear(2048, 1008)
        for p in self.parameters():
            p.requires_grad_(False)
        self._packs: Optional[Dict[str, tuple]] = None
        self._packs_key = None
        self._arena: Dict[str, torch.Tensor] = {}
        self.stage_hook: Optional[Callable[[str], None]] = None      # called with the stage's name after each stage of LAYER_TABLE is enqueued
        self.eval()

    # ---- parameters in --------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        state_dict = {k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
        return super().load_state_dict(state_dict, strict, **kw)

    @classmethod
    def from_checkpoint(cls, path, **kw) -> "InceptionV3Compat":
        """A plain state_dict file under torch-fidelity's names (its `pt_inception-2015-12-05` file is one)."""
        net = cls(**kw)
        net.load_state_dict(torch.load(path, map_location="cpu"))
        return net

    def conv_layers(self) -> List[Tuple[str, BasicConv2d]]:
        """The 94 conv -> BN -> ReLU layers under their state_dict prefixes, in definition order."""
        return [(n, m) for n, m in self.named_modules() if isinstance(m, BasicConv2d)]

    def refresh(self) -> None:
        """Drops the operand packs: the next call rebuilds them (needed only after a write that moves no `_version`, e.g. through `.data`)."""
        self._packs = self._packs_key = None

    # ---- the operands of the HIP route ----------------------------------------------------------------
    def _operands(self, device) -> Dict[str, tuple]:
        tensors = list(self.parameters()) + list(self.buffers())
        key = (str(device), tuple((t.data_ptr(), t._version) for t in tensors))
        if self._packs is not None and self._packs_key == key:
            return self._packs
        layers = self.conv_layers()
        if any(m.conv.weight.device != device for _, m in layers) or self.fc.weight.device != device:
            raise ValueError(f"InceptionV3Compat: input on {device}, parameters on {self.fc.weight.device}; move the module with .to(device)")
        # scale = gamma / sqrt(var + eps), shift = beta - mean * scale: f64 on the host, rounded once (one copy down per kind, one copy up)
        g, b, mu, var = (torch.cat([getattr(m.bn, k).detach().reshape(-1) for _, m in layers]).to("cpu", torch.float64)
                         for k in ("weight", "bias", "running_mean", "running_var"))
        scale = g / torch.sqrt(var + BN_EPS)
        shift = b - mu * scale
        ss = torch.stack([scale, shift]).to(torch.float32).to(device)
        packs, o = {}, 0
        for name, m in layers:
            packs[name] = (ops.pack_conv_weight_f32(m.conv.weight), ss[0, o:o + m.cout], ss[1, o:o + m.cout])
            o += m.cout
        packs["fc"] = (ops.pack_conv_weight_f32(self.fc.weight.detach().view(1008, 2048, 1, 1)), None, self.fc.bias.detach().contiguous())
        self._names = {id(m): n for n, m in layers}
        self._packs, self._packs_key = packs, key
        return packs

    def _buf(self, tag: str, shape, device) -> torch.Tensor:
        """A view of the arena's buffer `tag` (grown on demand, kept across calls; one stream: the passes of a call reuse the four buffers in order)."""
        n = 1
        for s in shape:
            n *= s
        buf = self._arena.get(tag)
        if buf is None or buf.numel() < n or buf.device != device:
            buf = torch.empty(n, dtype=torch.float32, device=device)
            self._arena[tag] = buf
        return buf[:n].view(*shape)

    def _conv(self, layer: BasicConv2d, x: torch.Tensor, out: torch.Tensor, off: int = 0) -> torch.Tensor:
        w, scale, shift = self._packs[self._names[id(layer)]]
        return ops.conv2d_f32(x, w, layer.kernel, layer.stride, layer.padding, scale, shift, True, out, off)

    def _hip_block(self, block, x: torch.Tensor, out_tag: str) -> torch.Tensor:
        b, h, w, c = x.shape
        plan = block.plan()
        ho, wo = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if plan[-1] == ["max2"] else (h, w)

        def width(branch):
            last = branch[-1]
            return c if isinstance(last, str) else sum(s.cout for s in last) if isinstance(last, tuple) else last.cout
        out = self._buf(out_tag, (b, ho, wo, sum(width(br) for br in plan)), x.device)
        off = 0
        for branch in plan:
            cur, flip = x, 0
            for step in branch[:-1]:
                if isinstance(step, str):
                    cur = ops.pool2d_f32(cur, _POOLS[step], self._buf(f"t{flip}", cur.shape, x.device))
                else:
                    cur = self._conv(step, cur, self._buf(f"t{flip}", (b, *step.out_hw(cur.shape[1], cur.shape[2]), step.cout), x.device))
                flip ^= 1
            last = branch[-1]
            if isinstance(last, str):
                ops.pool2d_f32(cur, _POOLS[last], out, off)
            else:
                o = off
                for step in (last if isinstance(last, tuple) else (last,)):
                    self._conv(step, cur, out, o)
                    o += step.cout
            off += width(branch)
        return out

    def _hip_pass(self, x: torch.Tensor, features: torch.Tensor, unbiased: Optional[torch.Tensor], biased: Optional[torch.Tensor]) -> None:
        """x: NHWC f32 [b, S, S, 3], normalised -> rows of features / logits_unbiased / logits."""
        dev, tag = x.device, 0
        for name, make in LAYER_TABLE:
            out_tag = "ab"[tag]
            if make is None:
                b, h, w, c = x.shape
                x = ops.pool2d_f32(x, ops.POOL_MAX_S2, self._buf(out_tag, (b, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c), dev))
            else:
                m = getattr(self, name)
                if isinstance(m, BasicConv2d):
                    x = self._conv(m, x, self._buf(out_tag, (x.shape[0], *m.out_hw(x.shape[1], x.shape[2]), m.cout), dev))
                else:
                    x = self._hip_block(m, x, out_tag)
            tag ^= 1
            if self.stage_hook is not None:
                self.stage_hook(name)                               # tools/bench_inception.py records a device event here
        ops.global_avgpool_f32(x, out=features)
        w, _, bias = self._packs["fc"]
        f = features.view(features.shape[0], 1, 1, 2048)
        if unbiased is not None:
            ops.conv2d_f32(f, w, (1, 1), out=unbiased.view(-1, 1, 1, 1008))
        if biased is not None:
            ops.conv2d_f32(f, w, (1, 1), shift=bias, out=biased.view(-1, 1, 1, 1008))

    def _check_input(self, x: torch.Tensor, dtype, what: str) -> None:
        if x.dtype != dtype or x.dim() != 4 or x.shape[1] != 3 or x.shape[0] == 0:
            raise TypeError(f"InceptionV3Compat.{what}: expected a non-empty {dtype} [B, 3, H, W], got {x.dtype} {tuple(x.shape)}")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError(f"InceptionV3Compat.{what}: inference only -- the input or a parameter requires a gradient and gradients are enabled; "
                               "call it under torch.no_grad() with parameters that do not require gradients")

    @torch.no_grad()
    def _run(self, x: torch.Tensor, want_unbiased: bool, want_biased: bool, chunk: Optional[int]):
        """x: uint8 or normalised f32 NCHW at the network's input size, on the GPU."""
        self._operands(x.device)
        n = x.shape[0]
        step = self.chunk if chunk is None else int(chunk)
        if step < 1:
            raise ValueError(f"chunk: expected >= 1, got {chunk}")
        features = torch.empty(n, 2048, dtype=torch.float32, device=x.device)
        unbiased = torch.empty(n, 1008, dtype=torch.float32, device=x.device) if want_unbiased else None
        biased = torch.empty(n, 1008, dtype=torch.float32, device=x.device) if want_biased else None
        for i in range(0, n, step):
            j = min(n, i + step)
            self._hip_pass(ops.inception_input(x[i:j]), features[i:j], None if unbiased is None else unbiased[i:j], None if biased is None else biased[i:j])
        return features, unbiased, biased

    # ---- the stock f32 composition -------------------------------------------------------------------
    @torch.no_grad()
    def forward_stock(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x f32 [B, 3, S, S], normalised -> (features, logits_unbiased) through F.conv2d / F.batch_norm / F.*_pool2d on the tensors' device."""
        for name, make in LAYER_TABLE:
            if make is None:
                x = F.max_pool2d(x, 3, 2)
            else:
                m = getattr(self, name)
                x = m(x) if isinstance(m, BasicConv2d) else _stock_block(m, x)
        features = x.mean(dim=(2, 3))
        return features, features.mm(self.fc.weight.t())

    # ---- the public calls ----------------------------------------------------------------------------
    def forward(self, u8: torch.Tensor, *, chunk: Optional[int] = None) -> torch.Tensor:
        """uint8 [B, 3, H, W] -> features f32 [B, 2048].  A size other than 299 x 299 goes through torch-fidelity's TF1-style bilinear resize first
        (`ops.resize_tf1_bilinear`), as its extractor does.  No host synchronisation."""
        self._check_input(u8, torch.uint8, "forward")
        resize = tuple(u8.shape[2:]) != (self.input_size, self.input_size)
        if not u8.is_cuda:
            _stock.require_opt_in("InceptionV3Compat.forward", "CPU images")
            from ..fidelity import _stock_resize_tf1_bilinear
            x = _stock_resize_tf1_bilinear(u8, self.input_size, False) if resize else (u8.float() - 128) / 128
            return self.forward_stock(x)[0]
        u8 = u8.contiguous()
        x = ops.resize_tf1_bilinear(u8, self.input_size, nhwc=False) if resize else u8
        return self._run(x, False, False, chunk)[0]

    def features_logits(self, x: torch.Tensor, *, biased: bool = False, chunk: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """x f32 [B, 3, S, S], S >= 75, already (resize(u8) - 128) / 128 -> (features f32 [B, 2048], logits f32 [B, 1008]): `logits_unbiased` = features
        fc.weight^T (what sample_50k.py asks for with feature_layer_isc='logits_unbiased'), or with biased=True `logits` = that + fc.bias."""
        self._check_input(x, torch.float32, "features_logits")
        if x.shape[2] < self.min_size or x.shape[3] < self.min_size:
            raise ValueError(f"InceptionV3Compat.features_logits: the network needs images of at least {self.min_size} x {self.min_size}, got "
                             f"{x.shape[2]} x {x.shape[3]}")
        if not x.is_cuda:
            _stock.require_opt_in("InceptionV3Compat.features_logits", "CPU images")
            features, logits = self.forward_stock(x)
            return features, logits + self.fc.bias if biased else logits
        features, unbiased, with_bias = self._run(x.contiguous(), not biased, biased, chunk)
        return features, with_bias if biased else unbiased

    def extractor(self, biased: bool = False) -> Callable[[torch.Tensor], Tuple[torch.Tensor, torch.Tensor]]:
        """The callable `fidelity.FidelityMetrics(extractor, num_features=2048)` takes."""
        return lambda x: self.features_logits(x, biased=biased)


def fid_module(weights_path):
    """A module object with `dmvae_amd.fid`'s names whose `FID` builds this network from `weights_path` where the reference's scripts ask for the int
    feature 2048 (`FID()`, evaluation/fid.py:51-56): what `run_on_mi355x.py --inception-weights=PATH` registers as `evaluation.fid`.  `dmvae_amd.fid.FID`
    itself is not changed; a module / callable `feature` passes through."""
    import types

    from .. import fid as _fid

    class FID(_fid.FID):
        __doc__ = _fid.FID.__doc__

        def __init__(self, feature=2048, *args, **kwargs):
            if isinstance(feature, int) and not isinstance(feature, bool):
                if feature != InceptionV3Compat.num_features:
                    raise ValueError(f"FID(feature={feature}): InceptionV3Compat gives the 2048 pool features only")
                feature = InceptionV3Compat.from_checkpoint(weights_path)
            super().__init__(feature, *args, **kwargs)

    mod = types.ModuleType("dmvae_amd.fid_inception", _fid.__doc__)
    for name in _fid.__all__:
        setattr(mod, name, getattr(_fid, name))
    mod.FID, mod.__all__, mod.inception_weights = FID, list(_fid.__all__), str(weights_path)
    return mod
