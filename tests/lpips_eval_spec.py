"""Not a test: an f64 CPU restatement of the evaluation LPIPS (evaluation/metrics.py:26-29: torchmetrics' LearnedPerceptualImagePatchSimilarity with
net_type='alex', reduction='mean') as a plain function of a parameter dict, written out step by step from the library's published definition and
independent of dmvae_amd/models/lpips_alex.py; `random_state_dict`, the seeded parameters the tests run it with; and the test image pairs.  The library
itself cannot be run where this package is developed, and neither weight file (torchvision's AlexNet, the LPIPS v0.1 lin heads) is on any such machine.

The definition: inputs [N, 3, H, W] in [-1, 1];  s = (x - shift) / scale per channel;  torchvision's AlexNet `features` tapped after each of its five
ReLUs;  per tap and pixel n = f / sqrt(eps + sum_c f_c^2), eps 1e-8;  d_l = mean_{h,w} sum_c w_{l,c} (n1_c - n2_c)^2;  per image v = sum_l d_l;  the
function returns the mean of v.

The random parameters: conv weights N(0, 2 / fan_in) (He: a ReLU keeps half of the second moment), biases N(0, 0.1^2), lin weights U(0, 1) / C (non-negative,
as the published heads are), all from one CPU torch.Generator -- the same values on every machine.  The image pairs: a uniform in [-1, 1] and
b = clamp(a + 0.2 N(0, 1), -1, 1), a distorted copy.  `check_alive` is the condition the tests rely on: at every tap at least a quarter of the activations are
positive, and every per-image value is positive and finite -- a trunk that died in its ReLUs, or a pair that is no pair, would make every comparison pass.
With this initialisation at 64 x 64 and 95 x 71 the smallest share over the taps is 0.45 - 0.46 and the values lie near 1e-3 (9.5e-4 ... 1.0e-3)."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-8
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
# (state_dict prefix, cin, cout, kernel, stride, padding, a 3 x 3 stride-2 max pool in front): torchvision's AlexNet.features[0 .. 11]
CONVS = (("net.slice1.0", 3, 64, 11, 4, 2, False), ("net.slice2.3", 64, 192, 5, 1, 2, True), ("net.slice3.6", 192, 384, 3, 1, 1, True),
         ("net.slice4.8", 384, 256, 3, 1, 1, False), ("net.slice5.10", 256, 256, 3, 1, 1, False))
CHANNELS = tuple(c[2] for c in CONVS)
LIN_KEYS = tuple(f"lin{k}.model.1.weight" for k in range(5))


def expected_state_dict_shapes():
    """The published module's parameter and buffer names (its second registration of the heads, `lins.*`, left out) -> shapes."""
    want = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    for name, cin, cout, k, _, _, _ in CONVS:
        want[f"{name}.weight"], want[f"{name}.bias"] = (cout, cin, k, k), (cout,)
    for key, c in zip(LIN_KEYS, CHANNELS):
        want[key] = (1, c, 1, 1)
    return want


def random_state_dict(seed=0):
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, cin, cout, k, _, _, _ in CONVS:
        sd[f"{name}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
        sd[f"{name}.bias"] = torch.randn(cout, generator=g) * 0.1
    for key, c in zip(LIN_KEYS, CHANNELS):
        sd[key] = torch.rand(1, c, 1, 1, generator=g) / c
    sd["scaling_layer.shift"] = torch.tensor(SHIFT).view(1, 3, 1, 1)
    sd["scaling_layer.scale"] = torch.tensor(SCALE).view(1, 3, 1, 1)
    return sd


def torchvision_layout(sd):
    """The same tensors as a torchvision AlexNet state_dict (`features.N.*` plus classifier tensors a loader must ignore) and a lin file."""
    trunk = {}
    for name, *_ in CONVS:
        idx = name.rsplit(".", 1)[1]
        trunk[f"features.{idx}.weight"], trunk[f"features.{idx}.bias"] = sd[f"{name}.weight"], sd[f"{name}.bias"]
    trunk["classifier.1.weight"], trunk["classifier.1.bias"] = torch.zeros(8, 8), torch.zeros(8)
    return trunk, {k: sd[k] for k in LIN_KEYS}


def image_pairs(n, h, w, seed=1):
    """-> (a, b) f32 [n, 3, h, w] in [-1, 1]: a uniform, b = clamp(a + 0.2 N(0, 1))."""
    g = torch.Generator().manual_seed(int(seed))
    a = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    b = (a + 0.2 * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1)
    return a, b


def scaled(x, dtype=torch.float64):
    """The ScalingLayer.  The constants are the f32 values the published buffers hold, widened."""
    shift, scale = torch.tensor(SHIFT).view(1, 3, 1, 1).to(dtype), torch.tensor(SCALE).view(1, 3, 1, 1).to(dtype)
    return (x.to(dtype) - shift) / scale


def trunk(sd, x, dtype=torch.float64):
    """x [B, 3, H, W] in [-1, 1] -> the five tapped feature maps, NCHW, in `dtype`."""
    t = scaled(x, dtype)
    taps = []
    for name, _, _, _, stride, pad, pool in CONVS:
        if pool:
            t = F.max_pool2d(t, 3, 2)
        t = F.relu(F.conv2d(t, sd[f"{name}.weight"].to(dtype), sd[f"{name}.bias"].to(dtype), stride, pad))
        taps.append(t)
    return taps


def head_level(f1, f2, lin, eps=EPS):
    """One level: f1, f2 [B, C, h, w], lin [C] -> [B], in the tensors' dtype."""
    n1 = f1 / torch.sqrt(eps + (f1 * f1).sum(dim=1, keepdim=True))
    n2 = f2 / torch.sqrt(eps + (f2 * f2).sum(dim=1, keepdim=True))
    d = (n1 - n2) ** 2 * lin.view(1, -1, 1, 1)
    return d.sum(dim=1).mean(dim=(1, 2))


def forward(sd, img1, img2, dtype=torch.float64, eps=EPS):
    """-> (per-image values [N], taps of img1, taps of img2) in `dtype` (f64: the specification; f32: the stock composition whose distance from the f64
    values is the tests' e_ref)."""
    t1, t2 = trunk(sd, img1, dtype), trunk(sd, img2, dtype)
    v = None
    for k, (f1, f2) in enumerate(zip(t1, t2)):
        d = head_level(f1, f2, sd[LIN_KEYS[k]].to(dtype).reshape(-1), eps)
        v = d if v is None else v + d
    return v, t1, t2


def check_alive(values, taps1, taps2):
    """-> (smallest share of positive activations over the taps of both images, smallest and largest per-image value)."""
    share = min((t > 0).double().mean().item() for t in list(taps1) + list(taps2))
    return share, values.min().item(), values.max().item()


def rel_l2(a, ref):
    """Per-image relative L2 error of a against ref (any [B, ...]) -> f64 [B]."""
    a, ref = a.double().cpu().flatten(1), ref.double().cpu().flatten(1)
    return (a - ref).norm(dim=1) / ref.norm(dim=1)
