"""The evaluation LPIPS on the CPU: the f64 specification (tests/lpips_eval_spec.py) against a plain nn.Sequential AlexNet built here, its liveness with the
seeded parameters, dmvae_amd.models.lpips_alex.LPIPSAlex's state_dict layout and its three load layouts, dmvae_amd.metrics.LPIPS (unconfigured, configured
on CPU tensors behind the stock opt-in, argument errors), `evaluate(..., lpips=net)` and the shadow.  The kernels are covered by
tests/test_gpu_lpips_eval.py, their entry points' validation by tests/test_lpips_eval_abi.py.  Neither the library nor a weight file is on any machine this
package is developed on: everything here runs on seeded random parameters."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

import lpips_eval_spec as S
from conftest import ROOT
from dmvae_amd import _lib, metrics
from dmvae_amd.models.lpips_alex import LPIPSAlex

U32 = 2.0 ** -24
SIZES = [(64, 64), (95, 71)]


@pytest.fixture(scope="module")
def sd():
    return S.random_state_dict(0)


@pytest.fixture(scope="module")
def net(sd):
    n = LPIPSAlex()
    n.load_state_dict(sd)
    return n


@pytest.fixture
def unconfigured(monkeypatch):
    monkeypatch.delenv("DMVAE_LPIPS_ALEX_WEIGHTS", raising=False)
    metrics.configure_lpips(None)
    yield
    metrics.configure_lpips(None)


# ---- the specification ------------------------------------------------------------------------------------------------------------------------
def sequential_alexnet(sd):
    """torchvision's AlexNet.features[0 .. 11] as written in its source, in f64, holding the parameters of `sd`."""
    f = nn.Sequential(nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2),
                      nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2),
                      nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(), nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(),
                      nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU()).double()
    for name, *_ in S.CONVS:
        idx = int(name.rsplit(".", 1)[1])
        with torch.no_grad():
            f[idx].weight.copy_(sd[f"{name}.weight"])
            f[idx].bias.copy_(sd[f"{name}.bias"])
    return f.eval()


@pytest.mark.parametrize("h,w", SIZES)
def test_spec_against_a_sequential_alexnet_and_alive(sd, h, w):
    """The spec's taps and values agree to 1e-12 with the nn.Sequential network tapped after layers 1, 4, 7, 9, 11 and a head written with explicit loops
    over the levels; and the liveness every later comparison rests on."""
    a, b = S.image_pairs(4, h, w)
    v, t1, t2 = S.forward(sd, a, b)
    feats = sequential_alexnet(sd)
    shift, scale = torch.tensor(S.SHIFT).double().view(1, 3, 1, 1), torch.tensor(S.SCALE).double().view(1, 3, 1, 1)
    want = torch.zeros(4, dtype=torch.float64)
    with torch.no_grad():
        xa, xb = (a.double() - shift) / scale, (b.double() - shift) / scale
        level = 0
        for idx, layer in enumerate(feats):
            xa, xb = layer(xa), layer(xb)
            if idx in (1, 4, 7, 9, 11):
                assert (xa - t1[level]).abs().max().item() <= 1e-12 and (xb - t2[level]).abs().max().item() <= 1e-12, level
                na = xa / (S.EPS + xa.pow(2).sum(1, keepdim=True)).sqrt()
                nb = xb / (S.EPS + xb.pow(2).sum(1, keepdim=True)).sqrt()
                lin = sd[S.LIN_KEYS[level]].double()
                want += nn.functional.conv2d((na - nb).pow(2), lin).mean(dim=(1, 2, 3))
                level += 1
    assert level == 5 and ((v - want).abs() <= 1e-12 * want.abs()).all()
    assert [tuple(t.shape[1:2]) for t in t1] == [(c,) for c in S.CHANNELS]
    share, lo, hi = S.check_alive(v, t1, t2)
    print(f"lpips spec {h} x {w}: positive share {share:.3f}, values {lo:.3e} .. {hi:.3e}")
    assert share >= 0.25 and lo > 0 and hi < float("inf")


# ---- naming and loading -----------------------------------------------------------------------------------------------------------------------
def test_state_dict_names_and_shapes_are_the_published_ones():
    n = LPIPSAlex()
    got = {k: tuple(v.shape) for k, v in n.state_dict().items()}
    assert got == S.expected_state_dict_shapes()
    assert got["net.slice1.0.weight"] == (64, 3, 11, 11) and got["net.slice2.3.weight"] == (192, 64, 5, 5) and got["lin2.model.1.weight"] == (1, 384, 1, 1)
    assert not any(p.requires_grad for p in n.parameters())
    assert all(torch.isnan(p).all() for p in n.parameters())            # nothing is silently random: unloaded is NaN
    assert torch.equal(n.scaling_layer.shift.flatten(), torch.tensor(S.SHIFT)) and torch.equal(n.scaling_layer.scale.flatten(), torch.tensor(S.SCALE))
    with pytest.raises(ValueError):
        LPIPSAlex(eps=0.0)


def test_three_load_layouts_and_aliases(sd, tmp_path):
    same = lambda m: all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    # 1. the published names, with the heads' second registration alongside, as the published module's own state_dict has them
    full = dict(sd)
    for k in range(5):
        full[f"lins.{k}.model.1.weight"] = sd[S.LIN_KEYS[k]]
    torch.save(full, tmp_path / "full.pth")
    assert same(LPIPSAlex.from_checkpoint(tmp_path / "full.pth"))
    # 2. the alias names alone, and no scaling_layer buffers
    alias = {k: v for k, v in sd.items() if not k.startswith("lin") and not k.startswith("scaling_layer")}
    for k in range(5):
        alias[f"lins.{k}.model.1.weight"] = sd[S.LIN_KEYS[k]]
    n = LPIPSAlex()
    res = n.load_state_dict(alias)
    assert same(n) and not res.missing_keys and not res.unexpected_keys
    # 3. a torchvision trunk (classifier tensors ignored) and a lin file
    trunk, lin = S.torchvision_layout(sd)
    torch.save(trunk, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "lin.pth")
    m = LPIPSAlex.from_checkpoints(tmp_path / "alexnet.pth", tmp_path / "lin.pth", eps=1e-6)
    assert same(m) and m.eps == 1e-6 and not any(p.requires_grad for p in m.parameters())
    # a missing tensor is a KeyError that names it; a scaling layer that is not the published one is refused
    for missing in ("net.slice4.8.bias", "lin3.model.1.weight"):
        with pytest.raises(KeyError, match=missing.replace(".", r"\.")):
            LPIPSAlex().load_state_dict({k: v for k, v in sd.items() if k != missing})
    torch.save(trunk, tmp_path / "only_trunk.pth")
    with pytest.raises(KeyError, match="lin0"):
        LPIPSAlex.from_checkpoint(tmp_path / "only_trunk.pth")
    with pytest.raises(ValueError, match="scaling_layer"):
        LPIPSAlex().load_state_dict(dict(sd, **{"scaling_layer.shift": torch.zeros(1, 3, 1, 1)}))


# ---- metrics.LPIPS ----------------------------------------------------------------------------------------------------------------------------
def test_unconfigured_and_unbuilt_net_types_raise(unconfigured):
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="AlexNet"):
        metrics.LPIPS(x, x)
    for net_type in ("vgg", "squeeze"):
        with pytest.raises(NotImplementedError, match="not built"):
            metrics.LPIPS(x, x, net_type=net_type)
    with pytest.raises(ValueError):
        metrics.LPIPS(x, x, net_type="resnet")


@pytest.mark.parametrize("h,w", SIZES)
def test_configured_on_cpu_tensors_matches_the_spec_to_f32_error(sd, net, unconfigured, allow_stock, h, w):
    """The stock f32 composition against the f64 specification.  The bound is not a measurement: the trunk is five convolutions, each a blocked f32 sum that
    adds a relative error of a few u = 2^-24 to a feature vector's L2 norm, and the head's normalised differences are formed in f32 from features that each
    carry that error, so the value of a pair whose differences are not small against the features (b is a 0.2-sigma distortion of a) stays within 64 u
    (3.8e-6), five orders below what a wrong tap, a missing bias or a wrong channel weight gives.  Measured here: 1e-8 ... 2e-7."""
    a, b = S.image_pairs(4, h, w)
    v64, _, _ = S.forward(sd, a, b)
    assert metrics.configure_lpips(net) is net and metrics.lpips_network() is net
    per = net(a, b)
    assert per.dtype == torch.float64 and tuple(per.shape) == (4,)
    rel = ((per - v64).abs() / v64).max().item()
    print(f"lpips stock f32 route {h} x {w}: value {v64.mean().item():.6e}, largest relative error {rel:.2e}")
    assert rel <= 64 * U32
    got = metrics.LPIPS(a, b)
    assert got.dtype == torch.float32 and got.dim() == 0 and got.device == a.device
    assert torch.equal(got, per.mean().float())
    assert torch.equal(metrics.LPIPS(a, b, net_type="alex"), got)
    assert metrics.LPIPS(a, a).item() == 0.0
    assert torch.equal(metrics.LPIPS(a.bfloat16(), b.bfloat16()), metrics.LPIPS(a.bfloat16().float(), b.bfloat16().float()))


def test_configure_by_path_and_by_environment(sd, unconfigured, allow_stock, tmp_path, monkeypatch):
    torch.save(sd, tmp_path / "w.pth")
    a, b = S.image_pairs(1, 64, 64)
    want = S.forward(sd, a, b)[0].mean().item()
    n = metrics.configure_lpips(str(tmp_path / "w.pth"))
    assert isinstance(n, LPIPSAlex) and abs(metrics.LPIPS(a, b).item() - want) <= 64 * U32 * want
    metrics.configure_lpips(None)
    with pytest.raises(NotImplementedError):
        metrics.LPIPS(a, b)
    monkeypatch.setenv("DMVAE_LPIPS_ALEX_WEIGHTS", str(tmp_path / "w.pth"))
    assert abs(metrics.LPIPS(a, b).item() - want) <= 64 * U32 * want
    assert metrics.lpips_network() is metrics.lpips_network()           # built once
    monkeypatch.delenv("DMVAE_LPIPS_ALEX_WEIGHTS")
    with pytest.raises(NotImplementedError, match="AlexNet"):
        metrics.LPIPS(a, b)
    trunk, lin = S.torchvision_layout(sd)
    torch.save(trunk, tmp_path / "t.pth")
    torch.save(lin, tmp_path / "l.pth")
    metrics.configure_lpips((tmp_path / "t.pth", tmp_path / "l.pth"))
    assert abs(metrics.LPIPS(a, b).item() - want) <= 64 * U32 * want


def test_argument_errors(net, unconfigured, allow_stock):
    metrics.configure_lpips(net)
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        metrics.LPIPS(x + 1.5, x)
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        metrics.LPIPS(x, x - 1.001)
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        metrics.LPIPS(x, x * float("nan"))
    for bad1, bad2 in ((x[:, :2], x[:, :2]), (x, x[:1]), (x[0], x[0]), (torch.zeros(2, 1, 64, 64), torch.zeros(2, 1, 64, 64)), (x[:0], x[:0])):
        with pytest.raises(ValueError):
            metrics.LPIPS(bad1, bad2)
    with pytest.raises(ValueError, match="at least 63"):
        metrics.LPIPS(torch.zeros(1, 3, 62, 64), torch.zeros(1, 3, 62, 64))
    assert metrics.LPIPS(torch.zeros(1, 3, 63, 63), torch.zeros(1, 3, 63, 63)).item() == 0.0


def test_cpu_tensors_need_the_stock_opt_in(net, unconfigured, monkeypatch):
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    metrics.configure_lpips(net)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(_lib.DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        metrics.LPIPS(x, x)
    with pytest.raises(_lib.DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        net(x, x)


# ---- evaluate(..., lpips=net) -----------------------------------------------------------------------------------------------------------------
class StubVAE(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def encode(self, x):
        return x * 0.5

    def decode(self, z):
        return z * 2.6                                                   # leaves [-1, 1]: evaluate clamps what it hands to the metric


def test_evaluate_reports_lpips_only_when_asked(sd, net, allow_stock):
    from dmvae_amd.evaluate import evaluate
    g = torch.Generator().manual_seed(5)
    imgs = torch.rand(6, 3, 64, 70, generator=g) * 2 - 1
    batches = [(b, torch.zeros(len(b), dtype=torch.long)) for b in imgs.split([1, 3, 2])]
    plain = evaluate(StubVAE(), batches, num_samples=8, device="cpu")
    with_lpips = evaluate(StubVAE(), batches, num_samples=8, device="cpu", lpips=net)
    both = evaluate(StubVAE(), batches, num_samples=8, device="cpu", ssim=True, lpips=net)
    assert "LPIPS" not in plain and set(with_lpips) == set(plain) | {"LPIPS"} and set(both) == set(plain) | {"LPIPS", "SSIM"}
    assert all(with_lpips[k] == plain[k] for k in plain) and both["LPIPS"] == with_lpips["LPIPS"]
    rec = (imgs * 1.3).clamp(-1, 1)
    want = S.forward(sd, rec, imgs)[0].sum().item() / 8                  # the sum over the images divided by num_samples, PSNR's convention
    assert want > 0 and abs(with_lpips["LPIPS"] - want) <= 64 * U32 * want


# ---- the shadow -------------------------------------------------------------------------------------------------------------------------------
def test_shadow_registers_the_configured_function(sd, tmp_path):
    """In a fresh interpreter: install_shadow(ref, metrics=True, lpips_weights=path) makes evaluation.metrics.LPIPS compute with the file's values; without
    the path it raises as before; lpips_weights without metrics is refused; the launcher's --lpips-weights=PATH implies --hip-metrics."""
    torch.save(sd, tmp_path / "w.pth")
    a, b = S.image_pairs(2, 64, 64)
    torch.save({"a": a, "b": b, "want": S.forward(sd, a, b)[0].mean()}, tmp_path / "case.pth")
    code = f"""
import sys, torch
sys.path.insert(0, {ROOT!r})
import run_on_mi355x as L
L.install_shadow(None, metrics=True)
from evaluation.metrics import LPIPS
case = torch.load({str(tmp_path / 'case.pth')!r})
try:
    LPIPS(case["a"], case["b"])
    raise SystemExit("unconfigured LPIPS computed")
except NotImplementedError:
    pass
L.install_shadow(None, metrics=True, lpips_weights={str(tmp_path / 'w.pth')!r})
from evaluation.metrics import LPIPS
import dmvae_amd.metrics
from dmvae_amd.models.lpips_alex import LPIPSAlex
assert LPIPS is dmvae_amd.metrics.LPIPS and isinstance(dmvae_amd.metrics.lpips_network(), LPIPSAlex)
got = LPIPS(case["a"], case["b"]).double()
assert abs(got - case["want"]) <= 64 * 2.0 ** -24 * case["want"], (got, case["want"])
try:
    L.install_shadow(None, lpips_weights="x")
except ValueError:
    print("OK")
"""
    env = {k: v for k, v in os.environ.items() if k not in ("DMVAE_HIP_METRICS", "DMVAE_LPIPS_ALEX_WEIGHTS")}
    r = subprocess.run([sys.executable, "-W", "ignore", "-c", code], capture_output=True, text=True, timeout=300, env=dict(env, DMVAE_ALLOW_STOCK="1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_on_mi355x.py"), f"--lpips-weights={tmp_path / 'w.pth'}", "--check"], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0 and "evaluation.metrics" in r.stdout and "dmvae_amd.metrics" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
