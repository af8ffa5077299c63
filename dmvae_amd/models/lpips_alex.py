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
composition (`forward_stock`) behind `DMVAE_ALLOW_STOCK=1`, like every other module (dmvae_amd/_stock.py).

Everything but the layer table and the two trunk walks is `LPIPSEval` (dmvae_amd/models/lpips_eval.py), shared with net_type 'vgg' and 'squeeze'."""
from __future__ import annotations

from typing import List

import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .lpips_eval import SCALE, SHIFT, LPIPSEval, _nan_

__all__ = ["LPIPSAlex", "TRUNK", "SHIFT", "SCALE"]

# (slice, index in torchvision's AlexNet.features, cin, cout, kernel, stride, padding, max pool in front)
TRUNK = (("slice1", 0, 3, 64, 11, 4, 2, False), ("slice2", 3, 64, 192, 5, 1, 2, True), ("slice3", 6, 192, 384, 3, 1, 1, True),
         ("slice4", 8, 384, 256, 3, 1, 1, False), ("slice5", 10, 256, 256, 3, 1, 1, False))


class LPIPSAlex(LPIPSEval):
    """Two [N, 3, H, W] image batches in [-1, 1] (f32 or bf16, H, W >= 63) -> per-image LPIPS values f64 [N].  eps: the normalisation's epsilon (the
    library's constructor argument, default 1e-8; > 0).  chunk: image pairs per pass of the network."""

    min_size, channels = 63, tuple(t[3] for t in TRUNK)
    _min_size_why = "its third convolution is given a 3 x 3 map at that size"
    _FEATURE_SLICE = {idx: name for name, idx, *_ in TRUNK}

    def __init__(self, eps: float = 1e-8, chunk: int = 64):
        super().__init__(eps, chunk)

    def _build_trunk(self) -> None:
        for name, idx, cin, cout, k, stride, pad, _ in TRUNK:
            s = nn.Module()
            s.add_module(str(idx), _nan_(nn.Conv2d(cin, cout, k, stride, pad)))
            self.net.add_module(name, s)

    def convs(self) -> List[nn.Conv2d]:
        return [getattr(getattr(self.net, name), str(idx)) for name, idx, *_ in TRUNK]

    def _hip_taps(self, a, b, packs, each) -> None:
        x = ops.lpips_input(a, b)
        for level, (_, _, _, _, k, stride, pad, pool) in enumerate(TRUNK):
            if pool:
                x = ops.pool2d_f32(x, ops.POOL_MAX_S2)
            w, bias = packs["conv"][level]
            x = ops.conv2d_f32(x, w, (k, k), stride, (pad, pad), None, bias, True)
            each(level, x)

    def _stock_taps(self, x):
        for (_, _, _, _, _, stride, pad, pool), conv in zip(TRUNK, self.convs()):
            if pool:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, conv.weight, conv.bias, stride, pad))
            yield x
