"""CPU: DinoDisc (dmvae_amd/models/dinodisc.py) against captures from the reference's own models/dinodisc.py + models/dinov2.py
(tools/capture_golden_dinodisc.py -> tests/golden/dinodisc_{small,branches,manifest}.npz): the state_dict and checkpoint formats, the plain-PyTorch route
`forward_stock` and the restatement tests/dinodisc_spec.py (q=None) at the bars tests/test_oracle_vit.py holds the same backbone to -- rel_err 2e-5 on outputs,
1e-4 on gradients and gradient norms --, the spectral norm's buffers, the gate in front of the stock route and the opt-in shadow.

The two conv biases in front of a BatchNormLocal have an analytically zero gradient (the norm removes the per-channel mean), so a relative comparison of them
compares rounding noise; they are bounded absolutely instead, against the gradient norm of the same conv's weight.  In the reference's own f32 capture
max |d bias| / ||d weight_orig|| is 2.1e-8, 4.9e-9, 8.6e-9 and 3.5e-9 for the four convs; the bar here is 1e-7 (five times the largest of them)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import dinodisc_spec as S
from conftest import ROOT, load_golden, rel_err

ZERO_GRAD_FACTOR = 1e-7


def zero_grad_bias(k):
    return k.endswith(".0.bias")            # heads.i.0.0.bias and heads.i.1.fn.0.bias (heads.i.2.bias is not in front of a norm)


@pytest.fixture
def area_branch(monkeypatch):
    monkeypatch.setattr(random, "random", lambda: 0.75)


def check_head_grads(g, grads):
    """grads: name -> gradient, against the capture's full / sliced / norm records."""
    for k, gr in grads.items():
        if zero_grad_bias(k):
            wk = k[:-4] + "weight_orig"
            assert gr.abs().max().item() <= ZERO_GRAD_FACTOR * float(g["gn." + wk]), k
        elif "g." + k in g:
            assert rel_err(gr, g.t("g." + k)) < 1e-4, k
        else:
            stride = 97 if gr.numel() < 200000 else 997
            assert rel_err(gr.flatten()[::stride], g.t("gs." + k)) < 1e-4, k
            assert abs(gr.double().norm().item() - float(g["gn." + k])) < 1e-4 * float(g["gn." + k]), k
            assert abs(gr.double().sum().item() - float(g["gsum." + k])) < 1e-4 * float(g["gn." + k]), k


def test_state_dict_and_checkpoint_formats(tmp_path):
    import warnings
    from dmvae_amd.models.dinodisc import DinoDisc
    m = load_golden("dinodisc_manifest")
    ckpt = S.filled_backbone({str(k): tuple(int(d) for d in s if d >= 0) for k, s in zip(m["ckpt_keys"], m["ckpt_shapes"])}, 3)
    assert "mask_token" in ckpt and ckpt["pos_embed"].shape == (1, 1370, 384)
    path = str(tmp_path / "dinov2_vits14.pth")
    torch.save(ckpt, path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # a checkpoint is given: no random-backbone warning
        disc = DinoDisc(9, "cpu", path)                      # strict load inside
    sd = disc.state_dict()
    assert list(sd.keys()) == [str(k) for k in m["disc_keys"]] and len(sd) == 66
    for k, s in zip(m["disc_keys"], m["disc_shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(d) for d in s if d >= 0), k
    assert torch.equal(disc.dino[0].pos_embed, ckpt["pos_embed"]) and not any(p.requires_grad for p in disc.dino[0].parameters())
    assert not disc.dino[0].training and not any(k.startswith("dino") for k in sd)
    with pytest.warns(UserWarning, match="randomly initialised"):
        DinoDisc(9, "cpu", None, dino_depth=1, key_depths=(0,))


def test_module_survives_copy_move_and_mode_changes(area_branch, allow_stock):
    import copy
    disc, _, _ = S.build_module(depth=2, key_depths=(0, 1), ks=3)
    x = S.image(2, 70, 1)
    disc.eval()
    with torch.no_grad():
        want = disc(x)
        twin = copy.deepcopy(disc)
        assert twin.dino[0] is not disc.dino[0] and torch.equal(twin(x), want)
        assert torch.equal(disc.to(torch.device("cpu")).requires_grad_(False).requires_grad_(True).train().eval()(x), want)
        assert torch.equal(disc(x, grad_ckpt=True), want)
    assert not disc.dino[0].training and all(p.requires_grad for p in disc.parameters())


def test_stock_route_train_mode_vs_reference(area_branch):
    g = load_golden("dinodisc_small")
    c = S.SMALL
    disc, _, heads = S.build_module()
    disc.train()
    logits = disc.forward_stock(S.image(c["batch"], c["px"], c["x_seed"]))
    assert logits.shape == (12, 648) and rel_err(logits.detach(), g.t("logits_train")) < 2e-5
    dy = torch.randn(logits.shape, generator=torch.Generator().manual_seed(c["dy_seed"]))
    (logits * dy).sum().backward()
    check_head_grads(g, {k: p.grad for k, p in disc.named_parameters()})
    sd = disc.state_dict()
    uv = [k for k in sd if k.endswith(("weight_u", "weight_v"))]
    assert len(uv) == 12
    for k in uv:                                             # one power iteration, v then u
        assert rel_err(sd[k], g.t("uv." + k)) < 2e-5, k
        assert sd[k].numel() == 1 or not torch.equal(sd[k], heads[k]), k          # (a one-element u is +-1 before and after)


def test_stock_route_eval_mode_input_gradient_vs_reference(area_branch):
    g = load_golden("dinodisc_small")
    c = S.SMALL
    disc, _, heads = S.build_module()
    disc.eval().requires_grad_(False)
    x = S.image(c["batch"], c["px"], c["x_seed"]).requires_grad_(True)
    logits = disc.forward_stock(x)
    assert rel_err(logits.detach(), g.t("logits_eval")) < 2e-5
    dy = torch.randn(logits.shape, generator=torch.Generator().manual_seed(c["dy_seed"]))
    (logits * dy).sum().backward()
    assert rel_err(x.grad[:, :, ::16, ::16], g.t("dx_slice")) < 1e-4
    assert abs(x.grad.double().norm().item() - float(g["dx_norm"])) < 1e-4 * float(g["dx_norm"])
    sd = disc.state_dict()
    assert all(torch.equal(sd[k], heads[k]) for k in sd if k.endswith(("weight_u", "weight_v")))       # eval: no power iteration


def branch_inputs(g):
    """(name, image, how to set the generators) for the three captured preprocessing branches."""
    def seed_crop():
        random.seed(int(g["crop_random_seed"]))
        torch.manual_seed(int(g["crop_torch_seed"]))
    return [("crop", S.image(2, 256, 7), seed_crop), ("px252", S.image(2, 252, 8), lambda: None), ("px70", S.image(2, 70, 9), lambda: None)]


def test_stock_route_preprocessing_branches_vs_reference():
    g = load_golden("dinodisc_branches")
    disc, _, _ = S.build_module()
    disc.eval()
    for name, x, seed in branch_inputs(g):
        seed()
        with torch.no_grad():
            out = disc.forward_stock(x)
        assert out.shape == g[name].shape and rel_err(out, g.t(name)) < 2e-5, name
    assert g["px70"].shape == (2, 2 * 25)                    # L = 25: shorter than the reach of the nine taps on both sides at once


def test_spec_twin_in_f32_vs_reference():
    g = load_golden("dinodisc_small")
    c = S.SMALL
    _, backbone, heads = S.build_module()
    x = S.image(c["batch"], c["px"], c["x_seed"])
    p = {k: v.clone().requires_grad_(not k.endswith(("weight_u", "weight_v"))) for k, v in heads.items()}
    uv = {}
    logits = S.forward(x, backbone, p, c["ks"], c["key_depths"], train=True, new_uv=uv)
    assert rel_err(logits.detach(), g.t("logits_train")) < 2e-5
    dy = torch.randn(logits.shape, generator=torch.Generator().manual_seed(c["dy_seed"]))
    (logits * dy).sum().backward()
    check_head_grads(g, {k: v.grad for k, v in p.items() if v.requires_grad})
    for k, v in uv.items():
        assert rel_err(v, g.t("uv." + k)) < 2e-5, k
    xe = x.clone().requires_grad_(True)
    le = S.forward(xe, backbone, heads, c["ks"], c["key_depths"], train=False)
    assert rel_err(le.detach(), g.t("logits_eval")) < 2e-5
    (le * dy).sum().backward()
    assert rel_err(xe.grad[:, :, ::16, ::16], g.t("dx_slice")) < 1e-4
    assert abs(xe.grad.double().norm().item() - float(g["dx_norm"])) < 1e-4 * float(g["dx_norm"])
    gb = load_golden("dinodisc_branches")
    with torch.no_grad():
        assert rel_err(S.forward(S.image(2, 70, 9), backbone, heads, c["ks"], c["key_depths"], train=False, branch="bicubic"), gb.t("px70")) < 2e-5


def test_gate_and_refusals(monkeypatch, area_branch):
    from dmvae_amd._lib import DmvaeHipError
    from dmvae_amd.models.dinodisc import DinoDisc
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    disc, _, _ = S.build_module(depth=1, key_depths=(0,), ks=3)
    with pytest.raises(DmvaeHipError, match="CPU tensor"):
        disc(S.image(2, 70, 1))
    with pytest.raises(NotImplementedError, match="dinodisc.py:62-65"):
        DinoDisc(9, "cpu", None, norm_type="sbn", dino_depth=1, key_depths=(0,))
    with pytest.raises(RuntimeError, match="9 does not split"):          # G = ceil(9 / 8) = 2 groups: the reference's view raises too
        disc.forward_stock(S.image(9, 70, 1))


def test_shadow_is_an_opt_in():
    """In a fresh interpreter: install_shadow(ref) still resolves DinoDisc to the reference's file, install_shadow(ref, dinodisc=True) -- and the command line's
    --hip-dinodisc / DMVAE_HIP_DINODISC=1 -- to this build's."""
    code = r"""
import sys, os, tempfile
sys.path.insert(0, %r)
import run_on_mi355x as L
ref = tempfile.mkdtemp()
os.makedirs(os.path.join(ref, "models"))
open(os.path.join(ref, "models", "dinodisc.py"), "w").write("class DinoDisc: marker = 'reference file'\n")
optin = sys.argv[1] == "1"
L.install_shadow(ref, dinodisc=True) if optin else L.install_shadow(ref)
from models import DinoDisc
from models.dinodisc import DinoDisc as D2
import dmvae_amd.models.dinodisc as ours
assert DinoDisc is D2
assert (DinoDisc is ours.DinoDisc) if optin else (DinoDisc.marker == 'reference file')
print("shadow ok")
""" % ROOT
    for optin in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code, optin], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "shadow ok" in r.stdout, r.stderr[-2000:]
    env = dict(os.environ, DMVAE_HIP_DINODISC="1")
    for argv, e in ((["--hip-dinodisc", "--check"], os.environ), (["--check"], env)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "run_on_mi355x.py")] + argv, capture_output=True, text=True, timeout=300, env=dict(e))
        assert r.returncode == 0 and "dmvae_amd.models.dinodisc" in r.stdout, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_on_mi355x.py"), "--check"], capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k != "DMVAE_HIP_DINODISC"})
    assert r.returncode == 0 and "dinodisc" not in r.stdout, r.stderr[-2000:]
