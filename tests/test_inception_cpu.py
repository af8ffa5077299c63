"""dmvae_amd.models.inception on the CPU: the state_dict layout (torch-fidelity's names), the load round trip, the f64 specification's per-stage shapes
and its liveness with the seeded parameters, the stock f32 route against the f64 specification (its distance is the e_ref of tests/test_gpu_inception.py),
the opt-in gate, and the two metric objects built around the module without torchmetrics."""
import pytest
import torch

import inception_spec as S
from dmvae_amd import _lib, ops
from dmvae_amd.fid import FID
from dmvae_amd.fidelity import FidelityMetrics
from dmvae_amd.models.inception import InceptionV3Compat

U = 2.0 ** -24


@pytest.fixture(scope="module")
def sd():
    return S.random_state_dict(0)


@pytest.fixture(scope="module")
def net(sd):
    n = InceptionV3Compat()
    n.load_state_dict(sd)
    return n


def test_state_dict_keys_and_shapes():
    got = {k: tuple(v.shape) for k, v in InceptionV3Compat().state_dict().items()}
    want = {}
    for name, cin, cout, (kh, kw), _, _ in S.LAYERS:
        want[f"{name}.conv.weight"] = (cout, cin, kh, kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            want[f"{name}.bn.{k}"] = (cout,)
    want["fc.weight"], want["fc.bias"] = (1008, 2048), (1008,)
    assert len(S.LAYERS) == 94 and len(want) == 94 * 5 + 2
    assert got == want
    assert got["Mixed_6c.branch7x7dbl_3.conv.weight"] == (160, 160, 1, 7)
    assert got["Mixed_7c.branch3x3dbl_1.conv.weight"] == (448, 2048, 1, 1)
    assert got["Conv2d_1a_3x3.conv.weight"] == (32, 3, 3, 3)
    assert got["Mixed_6a.branch3x3.conv.weight"] == (384, 288, 3, 3)
    assert got["Mixed_7b.branch3x3_2b.conv.weight"] == (384, 384, 3, 1)
    assert InceptionV3Compat.num_features == 2048 and InceptionV3Compat.num_classes == 1008


def test_load_state_dict_round_trip_tolerates_num_batches_tracked(sd, tmp_path):
    with_nbt = dict(sd)
    for name, *_ in S.LAYERS:
        with_nbt[f"{name}.bn.num_batches_tracked"] = torch.tensor(7)
    n = InceptionV3Compat()
    res = n.load_state_dict(with_nbt)
    assert not res.missing_keys and not res.unexpected_keys
    back = n.state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert not any(p.requires_grad for p in n.parameters())
    torch.save(with_nbt, tmp_path / "w.pth")
    m = InceptionV3Compat.from_checkpoint(tmp_path / "w.pth")
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        n.load_state_dict({k: v for k, v in sd.items() if k != "fc.bias"})


@pytest.mark.parametrize("size", [299, 139])
def test_spec_stage_shapes(sd, size):
    stages = {}
    f, lu, l = S.forward(sd, S.normalise(S.images(1, size)), stages=stages)
    sizes = S.stage_sizes(size)
    assert list(stages) == list(S.STAGES_299)
    for name, (s299, c) in S.STAGES_299.items():
        assert stages[name] == (1, c, sizes[name], sizes[name]), name
        if size == 299:
            assert sizes[name] == s299, name
    assert tuple(f.shape) == (1, 2048) and tuple(lu.shape) == (1, 1008) and tuple(l.shape) == (1, 1008)


@pytest.mark.parametrize("n,size", [(2, 299), (5, 139)])
def test_spec_is_alive_and_stock_route_matches_it(sd, net, allow_stock, n, size):
    """The condition every comparison with the specification rests on, then the module's CPU route (the stock f32 composition) against it.  e_ref, the
    per-image relative L2 distance of that f32 route from the f64 values, is printed: measured here 2.0e-7 (features) / 2.7e-7 (logits_unbiased) at 299 and
    3.6e-7 / 3.9e-7 at 139.  The bound on it is not a measurement: a path through the network crosses at most 22 conv layers, each a blocked f32 sum
    that contributes a relative error of a few u = 2^-24 to a vector's L2 norm, independent from layer to layer, so 64 u (3.8e-6) lies well above what such
    a composition can produce and five orders below what a wrong tap or a wrong concat order gives (a relative error near 1)."""
    u8 = S.images(n, size)
    f64, lu64, l64 = S.forward(sd, S.normalise(u8))
    share, lo, hi = S.check_alive(f64)
    assert share >= 0.5 and 1e-3 <= lo and hi <= 1e3, (share, lo, hi)
    x = S.normalise(u8).float()
    f, lu = net.features_logits(x)
    assert f.dtype == torch.float32 and tuple(f.shape) == (n, 2048) and tuple(lu.shape) == (n, 1008)
    e_f, e_l = S.rel_l2(f, f64).max().item(), S.rel_l2(lu, lu64).max().item()
    print(f"e_ref at {size}: features {e_f:.3e} logits_unbiased {e_l:.3e}")
    assert e_f <= 64 * U and e_l <= 64 * U
    _, lb = net.features_logits(x, biased=True)
    assert S.rel_l2(lb, l64).max().item() <= 64 * U
    if size == 299:
        assert torch.equal(net(u8), f)                                    # forward(u8) = the features of (u8 - 128) / 128
    else:
        from dmvae_amd.fidelity import _stock_resize_tf1_bilinear
        assert torch.equal(net(u8), net.features_logits(_stock_resize_tf1_bilinear(u8, 299, False))[0])


def test_cpu_input_raises_without_the_opt_in(net, monkeypatch):
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    with pytest.raises(_lib.DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        net(S.images(1, 299))
    with pytest.raises(_lib.DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
        net.features_logits(torch.zeros(1, 3, 299, 299))


def test_inference_only_and_input_checks(net, allow_stock):
    x = torch.zeros(1, 3, 75, 75, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        net.features_logits(x)
    with torch.no_grad():
        f, _ = net.features_logits(x)
    assert not f.requires_grad
    with pytest.raises(ValueError, match="at least 75"):
        net.features_logits(torch.zeros(1, 3, 74, 74))
    with pytest.raises(TypeError):
        net(torch.zeros(1, 3, 299, 299))
    with pytest.raises(TypeError):
        net.features_logits(torch.zeros(1, 3, 299, 299, dtype=torch.uint8))


def test_metric_objects_construct_around_the_module(net):
    fid = FID(feature=net)
    assert fid.num_features == 2048 and fid.inception is net
    fm = FidelityMetrics(net.extractor(), num_features=2048)
    assert fm.num_features == 2048 and fm.isc.num_classes == 1008
    with pytest.raises(ImportError):
        FID(feature=2048)                                                 # unchanged: the int form still asks for torchmetrics


def test_pack_conv_weight_f32_is_a_permutation():
    """Position 4 q + s of chunk c holds k = 16 c + 4 s + q of the (ky, kx, ci)-ordered K; Cin = 3 pads every tap to 4 channels and the taps to 12."""
    w = torch.arange(32 * 48 * 3 * 1, dtype=torch.float32).view(32, 48, 3, 1)
    p = ops.pack_conv_weight_f32(w)
    assert tuple(p.shape) == (9, 32, 16)
    k = w.permute(0, 2, 3, 1).reshape(32, -1)
    for c, q, s in ((0, 0, 0), (0, 1, 0), (0, 0, 1), (4, 3, 2), (8, 2, 3)):
        assert torch.equal(p[c, :, 4 * q + s], k[:, 16 * c + 4 * s + q])
    w3 = torch.randn(16, 3, 3, 3)
    p3 = ops.pack_conv_weight_f32(w3)
    assert tuple(p3.shape) == (3, 16, 16)
    flat = p3.view(3, 16, 4, 4).transpose(2, 3).permute(1, 0, 2, 3).reshape(16, 12, 4)      # [cout][tap][channel]
    assert torch.equal(flat[:, :9, :3], w3.permute(0, 2, 3, 1).reshape(16, 9, 3))
    assert flat[:, 9:].abs().sum() == 0 and flat[:, :, 3].abs().sum() == 0


def test_shadow_with_a_weight_file_builds_the_network_for_the_scripts_fid(sd, tmp_path):
    """install_shadow(ref, fid=True, inception_weights=path): `from evaluation.fid import FID; FID()` holds this build's network with the file's values;
    without the path the shadow stays dmvae_amd.fid (tests/test_fid_cpu.py).  In a fresh interpreter: the shadow edits sys.modules."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    torch.save(sd, tmp_path / "w.pth")
    code = f"""
import sys, torch
sys.path.insert(0, {ROOT!r})
import run_on_mi355x as L
L.install_shadow(None, fid=True, inception_weights={str(tmp_path / 'w.pth')!r})
from evaluation.fid import FID, frechet_distance
import dmvae_amd.fid
from dmvae_amd.models.inception import InceptionV3Compat
f = FID()
assert isinstance(f, dmvae_amd.fid.FID) and isinstance(f.inception, InceptionV3Compat) and f.num_features == 2048
w = torch.load({str(tmp_path / 'w.pth')!r})
assert torch.equal(f.inception.fc.weight, w["fc.weight"]) and torch.equal(f.inception.Mixed_7c.branch_pool.conv.weight, w["Mixed_7c.branch_pool.conv.weight"])
assert frechet_distance is dmvae_amd.fid.frechet_distance
try:
    L.install_shadow(None, inception_weights="x")
except ValueError:
    print("OK")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env={k: v for k, v in os.environ.items() if k != "DMVAE_HIP_FID"})
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_on_mi355x.py"), f"--inception-weights={tmp_path / 'w.pth'}", "--check"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "dmvae_amd.fid_inception" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
