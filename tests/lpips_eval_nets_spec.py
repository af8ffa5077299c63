"""Not a test: f64 CPU restatements of the evaluation LPIPS' net_type 'vgg' and 'squeeze' networks (evaluation/metrics.py:26-29 hands `net_type` to
torchmetrics' LearnedPerceptualImagePatchSimilarity) and of both normalisation forms, as plain functions of a parameter dict, written out layer by layer and
independent of dmvae_amd/models/lpips_eval.py; `random_state_dict(net, seed)`, the seeded parameters the tests run them with.  The image pairs,
`check_alive` and `rel_l2` are tests/lpips_eval_spec.py's.  Neither library nor any weight file is on a machine this package is developed on; the
SqueezeNet table is written from memory of the published definition.

'vgg': torchvision's vgg16.features (the reference's own table, utils/lpips.py:116-153), written here as the flat layer list -- 'C' a 3 x 3 padding-1
convolution and its ReLU (two indices), 'M' a 2 x 2 stride-2 max pool (one index) -- and tapped after indices 3, 8, 15, 22, 29.
'squeeze': torchvision's squeezenet1_1.features: 0 conv 3 -> 64 k3 s2, 1 ReLU, 2 pool(3, 2, ceil), 3 - 4 Fire, 5 pool, 6 - 7 Fire, 8 pool, 9 - 12 Fire;
tapped after indices 1, 4, 7, 9, 10, 11, 12.
Normalisation: form 0 n = f / sqrt(eps + sum_c f_c^2), eps 1e-8 (torchmetrics); form 1 n = f / (sqrt(sum_c f_c^2) + eps), eps 1e-10 (utils/lpips.py:156-158).

The random parameters: conv weights N(0, 2 / fan_in) (He), biases U(0, 0.1) -- small and positive, so that thirteen ReLUs in a row keep the trunk alive --
lin weights U(0, 1) / C, from one CPU torch.Generator.  `check_alive` (>= a quarter of every tap positive, every value finite and positive) was checked on
the CPU for every size the tests use before the seed was fixed (tests/test_lpips_eval_nets_cpu.py asserts it again): seed 0, smallest share over the
taps 0.47 (vgg; 16 x 16, 35 x 37, 64 x 48) and 0.48 (squeeze; 25 x 25, 35 x 37, 64 x 48), values 8.2e-4 ... 1.2e-3."""
import math

import torch
import torch.nn.functional as F

from lpips_eval_spec import SCALE, SHIFT, check_alive, image_pairs, rel_l2, scaled  # noqa: F401

EPS = {0: 1e-8, 1: 1e-10}

VGG_LAYERS = "CCMCCMCCCMCCCMCCC"
VGG_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
VGG_TAPS = (3, 8, 15, 22, 29)
VGG_SLICE_ENDS = (3, 8, 15, 22, 29)                    # the last features index of slice 1 .. 5
VGG_CHANNELS = (64, 128, 256, 512, 512)

# features index -> (cin, squeeze, expand1x1, expand3x3)
SQUEEZE_FIRES = {3: (64, 16, 64, 64), 4: (128, 16, 64, 64), 6: (128, 32, 128, 128), 7: (256, 32, 128, 128), 9: (256, 48, 192, 192),
                 10: (384, 48, 192, 192), 11: (384, 64, 256, 256), 12: (512, 64, 256, 256)}
SQUEEZE_POOLS = (2, 5, 8)
SQUEEZE_SLICE_ENDS = (1, 4, 7, 9, 10, 11, 12)          # = the taps
SQUEEZE_CHANNELS = (64, 128, 256, 384, 384, 512, 512)

CHANNELS = {"vgg": VGG_CHANNELS, "squeeze": SQUEEZE_CHANNELS}
MIN_SIZE = {"vgg": 16, "squeeze": 25}


def slice_of(ends, idx):
    return 1 + sum(idx > e for e in ends)


def vgg_convs():
    """-> [(features index, cin, cout)] by walking the layer list."""
    out, idx, cin, k = [], 0, 3, 0
    for layer in VGG_LAYERS:
        if layer == "M":
            idx += 1
        else:
            out.append((idx, cin, VGG_WIDTHS[k]))
            cin, k, idx = VGG_WIDTHS[k], k + 1, idx + 2
    return out


def conv_shapes(net):
    """-> {published name without .weight / .bias: (cout, cin, k)} of every convolution."""
    out = {}
    if net == "vgg":
        for idx, cin, cout in vgg_convs():
            out[f"net.slice{slice_of(VGG_SLICE_ENDS, idx)}.{idx}"] = (cout, cin, 3)
    else:
        out["net.slice1.0"] = (64, 3, 3)
        for idx, (cin, sq, e1, e3) in SQUEEZE_FIRES.items():
            p = f"net.slice{slice_of(SQUEEZE_SLICE_ENDS, idx)}.{idx}"
            out[f"{p}.squeeze"], out[f"{p}.expand1x1"], out[f"{p}.expand3x3"] = (sq, cin, 1), (e1, sq, 1), (e3, sq, 3)
    return out


def lin_keys(net):
    return tuple(f"lin{k}.model.1.weight" for k in range(len(CHANNELS[net])))


def expected_state_dict_shapes(net):
    want = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    for name, (cout, cin, k) in conv_shapes(net).items():
        want[f"{name}.weight"], want[f"{name}.bias"] = (cout, cin, k, k), (cout,)
    for key, c in zip(lin_keys(net), CHANNELS[net]):
        want[key] = (1, c, 1, 1)
    return want


def random_state_dict(net, seed=0):
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, (cout, cin, k) in conv_shapes(net).items():
        sd[f"{name}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
        sd[f"{name}.bias"] = torch.rand(cout, generator=g) * 0.1
    for key, c in zip(lin_keys(net), CHANNELS[net]):
        sd[key] = torch.rand(1, c, 1, 1, generator=g) / c
    sd["scaling_layer.shift"] = torch.tensor(SHIFT).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(SCALE).view(1, 3, 1, 1)
    return sd


def torchvision_layout(net, sd):
    """The same tensors as a torchvision state_dict (`features.N.*` plus classifier tensors a loader must ignore) and a lin file."""
    trunk = {}
    for k, v in sd.items():
        if k.startswith("net."):
            trunk["features." + k.split(".", 2)[2]] = v
    trunk["classifier.1.weight"], trunk["classifier.1.bias"] = torch.zeros(8, 8), torch.zeros(8)
    return trunk, {k: sd[k] for k in lin_keys(net)}


def _conv(sd, name, t, dtype, stride=1, pad=0):
    return F.relu(F.conv2d(t, sd[f"{name}.weight"].to(dtype), sd[f"{name}.bias"].to(dtype), stride, pad))


def trunk(net, sd, x, dtype=torch.float64):
    """x [B, 3, H, W] in [-1, 1] -> the tapped feature maps, NCHW, in `dtype`."""
    t, taps = scaled(x, dtype), []
    if net == "vgg":
        idx = 0
        for layer in VGG_LAYERS:
            if layer == "M":
                t, idx = F.max_pool2d(t, kernel_size=2, stride=2), idx + 1
            else:
                t, idx = _conv(sd, f"net.slice{slice_of(VGG_SLICE_ENDS, idx)}.{idx}", t, dtype, 1, 1), idx + 2
            if idx - 1 in VGG_TAPS:
                taps.append(t)
        return taps
    for idx in range(13):
        if idx == 0:
            t = _conv(sd, "net.slice1.0", t, dtype, 2, 0)
        elif idx in SQUEEZE_POOLS:
            t = F.max_pool2d(t, kernel_size=3, stride=2, ceil_mode=True)
        elif idx in SQUEEZE_FIRES:
            p = f"net.slice{slice_of(SQUEEZE_SLICE_ENDS, idx)}.{idx}"
            s = _conv(sd, f"{p}.squeeze", t, dtype)
            t = torch.cat([_conv(sd, f"{p}.expand1x1", s, dtype), _conv(sd, f"{p}.expand3x3", s, dtype, 1, 1)], dim=1)
        if idx in SQUEEZE_SLICE_ENDS:                  # index 1 is the ReLU of index 0, applied above
            taps.append(t)
    return taps


def head_level(f1, f2, lin, form=0, eps=None):
    """One level: f1, f2 [B, C, h, w], lin [C] -> [B], in the tensors' dtype."""
    eps = EPS[form] if eps is None else eps
    if form == 0:
        n1 = f1 / torch.sqrt(eps + (f1 * f1).sum(dim=1, keepdim=True))
        n2 = f2 / torch.sqrt(eps + (f2 * f2).sum(dim=1, keepdim=True))
    else:
        n1 = f1 / (torch.sqrt((f1 * f1).sum(dim=1, keepdim=True)) + eps)
        n2 = f2 / (torch.sqrt((f2 * f2).sum(dim=1, keepdim=True)) + eps)
    d = (n1 - n2) ** 2 * lin.view(1, -1, 1, 1)
    return d.sum(dim=1).mean(dim=(1, 2))


def forward(net, sd, img1, img2, dtype=torch.float64, form=0, eps=None):
    """-> (per-image values [N], taps of img1, taps of img2) in `dtype` (f64: the specification; f32: the stock composition whose distance from the f64
    values is the tests' e_ref)."""
    t1, t2 = trunk(net, sd, img1, dtype), trunk(net, sd, img2, dtype)
    v = None
    for key, f1, f2 in zip(lin_keys(net), t1, t2):
        d = head_level(f1, f2, sd[key].to(dtype).reshape(-1), form, eps)
        v = d if v is None else v + d
    return v, t1, t2
