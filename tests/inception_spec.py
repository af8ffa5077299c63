"""Not a test: an f64 CPU restatement of torch-fidelity's FeatureExtractorInceptionV3 (the network behind evaluation/fid.py:8-48 and
sample_50k.py:174-209) as a plain function of a parameter dict, written out layer by layer from the published definition and independent of
dmvae_amd/models/inception.py; `random_state_dict`, the seeded parameters the tests run it with (the published weights are on no machine this package is
developed on); and the test images.

The random parameters: conv weights N(0, 2 / fan_in) (He: a ReLU keeps half of the second moment), gamma ~ U(0.5, 1.5), beta ~ N(0, 0.1^2),
running_mean ~ N(0, 0.1^2), running_var ~ U(0.5, 1.5), fc weights N(0, 1 / 2048), fc bias N(0, 0.1^2), all from one CPU torch.Generator -- the same values
on every machine.  `check_alive` is the condition the tests rely on (tests/test_inception_cpu.py asserts it): for every test image at least half of the
2048 f64 features are non-zero and their rms lies in [1e-3, 1e3] -- a network that died through its 94 ReLUs would make every comparison pass."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-3
CONV_GAIN = 2.0            # conv weights ~ N(0, CONV_GAIN / fan_in)

# (prefix, cin, cout, (kh, kw), stride, (ph, pw)) of the 94 conv -> BN -> ReLU layers, in the order of the published module's definition


def _a(p, cin, pf):
    return [(f"{p}.branch1x1", cin, 64, (1, 1), 1, (0, 0)), (f"{p}.branch5x5_1", cin, 48, (1, 1), 1, (0, 0)), (f"{p}.branch5x5_2", 48, 64, (5, 5), 1, (2, 2)),
            (f"{p}.branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)), (f"{p}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
            (f"{p}.branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)), (f"{p}.branch_pool", cin, pf, (1, 1), 1, (0, 0))]


def _b(p, cin):
    return [(f"{p}.branch3x3", cin, 384, (3, 3), 2, (0, 0)), (f"{p}.branch3x3dbl_1", cin, 64, (1, 1), 1, (0, 0)),
            (f"{p}.branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)), (f"{p}.branch3x3dbl_3", 96, 96, (3, 3), 2, (0, 0))]


def _c(p, cin, c7):
    h, v = ((1, 7), 1, (0, 3)), ((7, 1), 1, (3, 0))
    return [(f"{p}.branch1x1", cin, 192, (1, 1), 1, (0, 0)), (f"{p}.branch7x7_1", cin, c7, (1, 1), 1, (0, 0)), (f"{p}.branch7x7_2", c7, c7, *h),
            (f"{p}.branch7x7_3", c7, 192, *v), (f"{p}.branch7x7dbl_1", cin, c7, (1, 1), 1, (0, 0)), (f"{p}.branch7x7dbl_2", c7, c7, *v),
            (f"{p}.branch7x7dbl_3", c7, c7, *h), (f"{p}.branch7x7dbl_4", c7, c7, *v), (f"{p}.branch7x7dbl_5", c7, 192, *h),
            (f"{p}.branch_pool", cin, 192, (1, 1), 1, (0, 0))]


def _d(p, cin):
    return [(f"{p}.branch3x3_1", cin, 192, (1, 1), 1, (0, 0)), (f"{p}.branch3x3_2", 192, 320, (3, 3), 2, (0, 0)),
            (f"{p}.branch7x7x3_1", cin, 192, (1, 1), 1, (0, 0)), (f"{p}.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
            (f"{p}.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), (f"{p}.branch7x7x3_4", 192, 192, (3, 3), 2, (0, 0))]


def _e(p, cin):
    h, v = ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0))
    return [(f"{p}.branch1x1", cin, 320, (1, 1), 1, (0, 0)), (f"{p}.branch3x3_1", cin, 384, (1, 1), 1, (0, 0)), (f"{p}.branch3x3_2a", 384, 384, *h),
            (f"{p}.branch3x3_2b", 384, 384, *v), (f"{p}.branch3x3dbl_1", cin, 448, (1, 1), 1, (0, 0)), (f"{p}.branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),
            (f"{p}.branch3x3dbl_3a", 384, 384, *h), (f"{p}.branch3x3dbl_3b", 384, 384, *v), (f"{p}.branch_pool", cin, 192, (1, 1), 1, (0, 0))]


LAYERS = ([("Conv2d_1a_3x3", 3, 32, (3, 3), 2, (0, 0)), ("Conv2d_2a_3x3", 32, 32, (3, 3), 1, (0, 0)), ("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)),
           ("Conv2d_3b_1x1", 64, 80, (1, 1), 1, (0, 0)), ("Conv2d_4a_3x3", 80, 192, (3, 3), 1, (0, 0))]
          + _a("Mixed_5b", 192, 32) + _a("Mixed_5c", 256, 64) + _a("Mixed_5d", 288, 64) + _b("Mixed_6a", 288)
          + _c("Mixed_6b", 768, 128) + _c("Mixed_6c", 768, 160) + _c("Mixed_6d", 768, 160) + _c("Mixed_6e", 768, 192)
          + _d("Mixed_7a", 768) + _e("Mixed_7b", 1280) + _e("Mixed_7c", 2048))
GEOMETRY = {name: (stride, pad) for name, _, _, _, stride, pad in LAYERS}

# stage -> (spatial size at a 299 input, channels): the table of the network's definition
STAGES_299 = {"Conv2d_1a_3x3": (149, 32), "Conv2d_2a_3x3": (147, 32), "Conv2d_2b_3x3": (147, 64), "MaxPool_1": (73, 64), "Conv2d_3b_1x1": (73, 80),
              "Conv2d_4a_3x3": (71, 192), "MaxPool_2": (35, 192), "Mixed_5b": (35, 256), "Mixed_5c": (35, 288), "Mixed_5d": (35, 288), "Mixed_6a": (17, 768),
              "Mixed_6b": (17, 768), "Mixed_6c": (17, 768), "Mixed_6d": (17, 768), "Mixed_6e": (17, 768), "Mixed_7a": (8, 1280), "Mixed_7b": (8, 2048),
              "Mixed_7c": (8, 2048)}


def stage_sizes(s):
    """The spatial size after every stage for an s x s input, by the stages' own arithmetic (valid 3x3: -2; stride 2: (n - 3) // 2 + 1)."""
    out = {}
    n = (s - 3) // 2 + 1
    out["Conv2d_1a_3x3"] = n
    n -= 2
    out["Conv2d_2a_3x3"] = out["Conv2d_2b_3x3"] = n
    n = (n - 3) // 2 + 1
    out["MaxPool_1"] = out["Conv2d_3b_1x1"] = n
    n -= 2
    out["Conv2d_4a_3x3"] = n
    n = (n - 3) // 2 + 1
    out["MaxPool_2"] = out["Mixed_5b"] = out["Mixed_5c"] = out["Mixed_5d"] = n
    n = (n - 3) // 2 + 1
    for k in ("Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        out[k] = n
    n = (n - 3) // 2 + 1
    out["Mixed_7a"] = out["Mixed_7b"] = out["Mixed_7c"] = n
    return out


def random_state_dict(seed=0, conv_gain=CONV_GAIN):
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for name, cin, cout, (kh, kw), _, _ in LAYERS:
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(conv_gain / (cin * kh * kw))
        sd[f"{name}.bn.weight"] = torch.rand(cout, generator=g) + 0.5
        sd[f"{name}.bn.bias"] = torch.randn(cout, generator=g) * 0.1
        sd[f"{name}.bn.running_mean"] = torch.randn(cout, generator=g) * 0.1
        sd[f"{name}.bn.running_var"] = torch.rand(cout, generator=g) + 0.5
    sd["fc.weight"] = torch.randn(1008, 2048, generator=g) * math.sqrt(1.0 / 2048)
    sd["fc.bias"] = torch.randn(1008, generator=g) * 0.1
    return sd


def images(n, size, seed=1):
    """uint8 [n, 3, size, size]: seeded uniform noise, the last image a smooth gradient (three different ramps)."""
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randint(0, 256, (n, 3, size, size), generator=g, dtype=torch.uint8)
    r = torch.arange(size, dtype=torch.float64) / (size - 1)
    ramp = torch.stack([r.view(-1, 1).expand(size, size), r.view(1, -1).expand(size, size), (r.view(-1, 1) + r.view(1, -1)) / 2])
    x[-1] = (ramp * 255).round().to(torch.uint8)
    return x


def normalise(u8):
    return (u8.double() - 128) / 128


def forward(sd, x, dtype=torch.float64, stages=None):
    """x [B, 3, S, S], normalised -> (features [B, 2048], logits_unbiased [B, 1008], logits [B, 1008]) in `dtype` (f64: the specification; f32: the stock
    composition whose distance from the f64 values is the tests' e_ref).  `stages`: a dict that receives every stage's output shape."""
    p = {k: v.to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    x = x.to(dtype)

    def cbr(name, t):
        stride, pad = GEOMETRY[name]
        t = F.conv2d(t, p[f"{name}.conv.weight"], None, stride, pad)
        t = F.batch_norm(t, p[f"{name}.bn.running_mean"], p[f"{name}.bn.running_var"], p[f"{name}.bn.weight"], p[f"{name}.bn.bias"], False, 0.0, EPS)
        return F.relu(t)

    def chain(prefix, names, t):
        for n in names:
            t = cbr(f"{prefix}.{n}", t)
        return t

    def avg(t):
        return F.avg_pool2d(t, 3, 1, 1, count_include_pad=False)

    def block_a(q, t):
        return torch.cat([cbr(f"{q}.branch1x1", t), chain(q, ("branch5x5_1", "branch5x5_2"), t),
                          chain(q, ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), t), cbr(f"{q}.branch_pool", avg(t))], 1)

    def block_b(q, t):
        return torch.cat([cbr(f"{q}.branch3x3", t), chain(q, ("branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), t), F.max_pool2d(t, 3, 2)], 1)

    def block_c(q, t):
        return torch.cat([cbr(f"{q}.branch1x1", t), chain(q, ("branch7x7_1", "branch7x7_2", "branch7x7_3"), t),
                          chain(q, ("branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"), t),
                          cbr(f"{q}.branch_pool", avg(t))], 1)

    def block_d(q, t):
        return torch.cat([chain(q, ("branch3x3_1", "branch3x3_2"), t), chain(q, ("branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"), t),
                          F.max_pool2d(t, 3, 2)], 1)

    def block_e(q, t, pool):
        b3 = cbr(f"{q}.branch3x3_1", t)
        bd = chain(q, ("branch3x3dbl_1", "branch3x3dbl_2"), t)
        return torch.cat([cbr(f"{q}.branch1x1", t), cbr(f"{q}.branch3x3_2a", b3), cbr(f"{q}.branch3x3_2b", b3), cbr(f"{q}.branch3x3dbl_3a", bd),
                          cbr(f"{q}.branch3x3dbl_3b", bd), cbr(f"{q}.branch_pool", pool(t))], 1)

    program = [("Conv2d_1a_3x3", lambda t: cbr("Conv2d_1a_3x3", t)), ("Conv2d_2a_3x3", lambda t: cbr("Conv2d_2a_3x3", t)),
               ("Conv2d_2b_3x3", lambda t: cbr("Conv2d_2b_3x3", t)), ("MaxPool_1", lambda t: F.max_pool2d(t, 3, 2)),
               ("Conv2d_3b_1x1", lambda t: cbr("Conv2d_3b_1x1", t)), ("Conv2d_4a_3x3", lambda t: cbr("Conv2d_4a_3x3", t)),
               ("MaxPool_2", lambda t: F.max_pool2d(t, 3, 2)),
               ("Mixed_5b", lambda t: block_a("Mixed_5b", t)), ("Mixed_5c", lambda t: block_a("Mixed_5c", t)), ("Mixed_5d", lambda t: block_a("Mixed_5d", t)),
               ("Mixed_6a", lambda t: block_b("Mixed_6a", t)),
               ("Mixed_6b", lambda t: block_c("Mixed_6b", t)), ("Mixed_6c", lambda t: block_c("Mixed_6c", t)), ("Mixed_6d", lambda t: block_c("Mixed_6d", t)),
               ("Mixed_6e", lambda t: block_c("Mixed_6e", t)), ("Mixed_7a", lambda t: block_d("Mixed_7a", t)),
               ("Mixed_7b", lambda t: block_e("Mixed_7b", t, avg)), ("Mixed_7c", lambda t: block_e("Mixed_7c", t, lambda u: F.max_pool2d(u, 3, 1, 1)))]
    for name, fn in program:
        x = fn(x)
        if stages is not None:
            stages[name] = tuple(x.shape)
    features = x.mean(dim=(2, 3))
    unbiased = features @ p["fc.weight"].t()
    return features, unbiased, unbiased + p["fc.bias"]


def check_alive(features):
    """-> (smallest share of non-zero features over the images, smallest and largest per-image feature rms)."""
    f = features.double()
    share = (f != 0).double().mean(dim=1).min().item()
    rms = f.pow(2).mean(dim=1).sqrt()
    return share, rms.min().item(), rms.max().item()


def rel_l2(a, ref):
    """Per-image relative L2 error of a against ref -> f64 [B]."""
    a, ref = a.double().cpu(), ref.double().cpu()
    return (a - ref).norm(dim=1) / ref.norm(dim=1)
