"""The evaluation LPIPS' 'vgg' and 'squeeze' networks on the CPU: the liveness of the f64 specification (tests/lpips_eval_nets_spec.py) with the seeded
parameters at every size the GPU tests use, dmvae_amd.models.lpips_eval.LPIPSVGG / LPIPSSqueeze's state_dict layouts, load aliases and `from_training`,
`metrics.configure_lpips` per type, the stock f32 composition against the f64 specification, `evaluate(..., lpips=net)` and the launcher's two flags.  The
kernels are covered by tests/test_gpu_lpips_eval_nets.py, their entry points' validation by tests/test_lpips_eval_nets_abi.py.  Neither library nor a
weight file is on any machine this package is developed on: everything here runs on seeded random parameters."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

import lpips_eval_nets_spec as N
import lpips_eval_spec as S
from conftest import ROOT
from dmvae_amd import metrics
from dmvae_amd.models.lpips_alex import LPIPSAlex
from dmvae_amd.models.lpips_eval import LPIPSEval, LPIPSSqueeze, LPIPSVGG

U32 = 2.0 ** -24
CLASSES = {"vgg": LPIPSVGG, "squeeze": LPIPSSqueeze}
SIZES = {"vgg": [(16, 16), (35, 37), (64, 48)], "squeeze": [(25, 25), (35, 37), (64, 48)]}
# convolutions on the longest path to the last tap: the stock route's bound below scales with it (AlexNet: 5)
DEPTH = {"vgg": 13, "squeeze": 17}
ENV = ("DMVAE_LPIPS_ALEX_WEIGHTS", "DMVAE_LPIPS_VGG_WEIGHTS", "DMVAE_LPIPS_SQUEEZE_WEIGHTS")
NETS = ("vgg", "squeeze")


@pytest.fixture(scope="module")
def sds():
    return {net: N.random_state_dict(net, 0) for net in NETS}


@pytest.fixture(scope="module")
def nets(sds):
    out = {}
    for net in NETS:
        out[net] = CLASSES[net]()
        out[net].load_state_dict(sds[net])
    return out


@pytest.fixture
def unconfigured(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    metrics.configure_lpips(None)
    yield
    metrics.configure_lpips(None)


# ---- the specification ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS)
def test_spec_is_alive_at_every_size_the_gpu_tests_use(sds, net):
    """At least a quarter of every tap positive and every value finite and positive (S.check_alive's condition): a dead tap would let a wrong layer pass."""
    for h, w in SIZES[net]:
        a, b = N.image_pairs(3, h, w)
        for form in ((0, 1) if net == "vgg" else (0,)):
            v, t1, t2 = N.forward(net, sds[net], a, b, form=form)
            share, lo, hi = N.check_alive(v, t1, t2)
            print(f"lpips {net} spec {h} x {w} form {form}: positive share {share:.3f}, values {lo:.3e} .. {hi:.3e}")
            assert share >= 0.25 and lo > 0 and hi < float("inf")
            assert [t.shape[1] for t in t1] == list(N.CHANNELS[net])
    assert SIZES[net][0] == (N.MIN_SIZE[net],) * 2 == (CLASSES[net].min_size,) * 2
    # the smallest size leaves the last tap one pixel
    assert tuple(N.trunk(net, sds[net], torch.zeros(1, 3, *SIZES[net][0]))[-1].shape[2:]) == (1, 1)


def test_vgg_table_is_the_training_loss_own():
    """The spec's layer list, the module's table and dmvae_amd.utils.lpips.vgg16 (the reference's own slices, utils/lpips.py:116-153) name the same
    thirteen convolutions."""
    from dmvae_amd.utils.lpips import vgg16
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = vgg16(pretrained=False)
    want = {f"net.{k}": tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: v for k, v in N.expected_state_dict_shapes("vgg").items() if k.startswith("net.")}
    assert got == want and len(got) == 26
    assert {k: tuple(v.shape) for k, v in LPIPSVGG().state_dict().items() if k.startswith("net.")} == want


def test_squeeze_min_size_is_derived_and_is_25():
    """Every pool must see at least 3 rows: conv k3 s2 leaves (s - 3) // 2 + 1, a ceil_mode pool ceil((h - 3) / 2) + 1.  24 -> 11 -> 5 -> 2: the third pool
    is short; 25 -> 12 -> 6 -> 3 -> 1."""
    def maps(s):
        out = [(s - 3) // 2 + 1]
        for _ in range(3):
            out.append(-(-(out[-1] - 3) // 2) + 1)
        return out
    assert maps(25) == [12, 6, 3, 1] and maps(24)[:3] == [11, 5, 2]
    assert LPIPSSqueeze.min_size == 25 == min(s for s in range(3, 64) if min(maps(s)[:3]) >= 3)
    assert LPIPSVGG.min_size == 16 and LPIPSAlex.min_size == 63


# ---- naming and loading -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS)
def test_state_dict_names_and_shapes_are_the_published_ones(net):
    n = CLASSES[net]()
    got = {k: tuple(v.shape) for k, v in n.state_dict().items()}
    assert got == N.expected_state_dict_shapes(net)
    assert n.channels == N.CHANNELS[net] and len(n.lins()) == len(N.CHANNELS[net])
    assert not any(p.requires_grad for p in n.parameters())
    assert all(torch.isnan(p).all() for p in n.parameters())            # nothing is silently random: unloaded is NaN
    assert torch.equal(n.scaling_layer.shift.flatten(), torch.tensor(S.SHIFT)) and torch.equal(n.scaling_layer.scale.flatten(), torch.tensor(S.SCALE))
    assert isinstance(n, LPIPSEval) and isinstance(LPIPSAlex(), LPIPSEval)
    with pytest.raises(ValueError):
        CLASSES[net](eps=0.0)
    with pytest.raises(ValueError):
        CLASSES[net](chunk=0)


def test_names_spelled_out():
    v, s = LPIPSVGG().state_dict(), LPIPSSqueeze().state_dict()
    assert tuple(v["net.slice1.2.weight"].shape) == (64, 64, 3, 3) and tuple(v["net.slice3.14.bias"].shape) == (256,)
    assert tuple(v["net.slice5.28.weight"].shape) == (512, 512, 3, 3) and tuple(v["lin4.model.1.weight"].shape) == (1, 512, 1, 1)
    assert tuple(s["net.slice1.0.weight"].shape) == (64, 3, 3, 3) and tuple(s["net.slice2.3.squeeze.weight"].shape) == (16, 64, 1, 1)
    assert tuple(s["net.slice4.9.expand3x3.weight"].shape) == (192, 48, 3, 3) and tuple(s["net.slice7.12.expand1x1.bias"].shape) == (256,)
    assert tuple(s["lin6.model.1.weight"].shape) == (1, 512, 1, 1) and "lin7.model.1.weight" not in s
    with pytest.raises(ValueError, match="normalize"):
        LPIPSVGG(normalize="lpips")
    assert LPIPSVGG().eps == 1e-8 and LPIPSVGG(normalize="reference").eps == 1e-10 and LPIPSVGG(normalize="reference", eps=1e-6).eps == 1e-6


@pytest.mark.parametrize("net", NETS)
def test_three_load_layouts_and_aliases(sds, net, tmp_path):
    sd, cls, keys = sds[net], CLASSES[net], N.lin_keys(net)
    same = lambda m: all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    full = dict(sd)
    for k, key in enumerate(keys):
        full[f"lins.{k}.model.1.weight"] = sd[key]
    torch.save(full, tmp_path / "full.pth")
    assert same(cls.from_checkpoint(tmp_path / "full.pth"))
    alias = {k: v for k, v in sd.items() if not k.startswith("lin") and not k.startswith("scaling_layer")}
    for k, key in enumerate(keys):
        alias[f"lins.{k}.model.1.weight"] = sd[key]
    n = cls()
    res = n.load_state_dict(alias)
    assert same(n) and not res.missing_keys and not res.unexpected_keys
    trunk, lin = N.torchvision_layout(net, sd)
    assert all(k.startswith(("features.", "classifier.")) for k in trunk) and len(trunk) == len([k for k in sd if k.startswith("net.")]) + 2
    torch.save(trunk, tmp_path / "trunk.pth")
    torch.save(lin, tmp_path / "lin.pth")
    m = cls.from_checkpoints(tmp_path / "trunk.pth", tmp_path / "lin.pth", eps=1e-6)
    assert same(m) and m.eps == 1e-6 and not any(p.requires_grad for p in m.parameters())
    last_conv = [k for k in sd if k.startswith("net.") and k.endswith(".bias")][-1]
    for missing in (last_conv, keys[-1], keys[0]):
        with pytest.raises(KeyError, match=missing.replace(".", r"\.")):
            cls().load_state_dict({k: v for k, v in sd.items() if k != missing})
    with pytest.raises(KeyError, match="lin0"):
        cls.from_checkpoint(tmp_path / "trunk.pth")
    with pytest.raises(ValueError, match="scaling_layer"):
        cls().load_state_dict(dict(sd, **{"scaling_layer.shift": torch.zeros(1, 3, 1, 1)}))
    with pytest.raises(KeyError, match=cls.__name__):
        cls().load_state_dict({})


def training_module(seed=0):
    """A dmvae_amd.utils.lpips.LPIPS holding seeded parameters, as tests/test_gpu_lpips.py builds it; the seeded trunk stands in for a loaded one."""
    from dmvae_amd.utils.lpips import LPIPS
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(seed)
        lp = LPIPS().eval()
    with torch.no_grad():
        for m in lp.net.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.normal_(0, (2.0 / (9 * m.weight.shape[1])) ** 0.5)
                m.bias.normal_(0, 0.05)
        for lin in (lp.lin0, lp.lin1, lp.lin2, lp.lin3, lp.lin4):
            lin.model[-1].weight.uniform_(0.0, 2.0 / lin.model[-1].weight.shape[1])
    return lp


def test_from_training_round_trip():
    lp = training_module()
    with pytest.raises(ValueError, match="trunk"):
        LPIPSVGG.from_training(lp)
    lp.net.trunk_loaded = True
    net = LPIPSVGG.from_training(lp, normalize="reference")
    assert net.head_form == 1 and net.eps == 1e-10 and LPIPSVGG.from_training(lp).head_form == 0
    theirs, ours = lp.state_dict(), net.state_dict()
    assert set(theirs) == set(ours) and all(torch.equal(theirs[k], ours[k]) for k in ours)
    assert all(ours[k].data_ptr() != theirs[k].data_ptr() for k in ours if not k.startswith("scaling_layer"))      # copies
    back = training_module(1)
    back.load_state_dict(net.state_dict())                               # and the training module takes the evaluation module's state_dict
    assert all(torch.equal(back.state_dict()[k], theirs[k]) for k in theirs)


# ---- metrics.LPIPS ----------------------------------------------------------------------------------------------------------------------------
def test_configure_lpips_keeps_one_network_per_type(nets, sds, unconfigured, allow_stock, tmp_path):
    alex = LPIPSAlex()
    alex.load_state_dict(S.random_state_dict(0))
    assert metrics.configure_lpips(nets["vgg"]) is nets["vgg"]           # a module selects its type
    assert metrics.lpips_network("vgg") is nets["vgg"] and metrics.lpips_network("squeeze") is None and metrics.lpips_network() is None
    metrics.configure_lpips(nets["squeeze"], net_type="squeeze")
    metrics.configure_lpips(alex)
    assert [metrics.lpips_network(t) for t in ("alex", "vgg", "squeeze")] == [alex, nets["vgg"], nets["squeeze"]]
    with pytest.raises(ValueError, match="net_type"):
        metrics.configure_lpips(nets["vgg"], net_type="squeeze")
    with pytest.raises(ValueError):
        metrics.configure_lpips(nets["vgg"], net_type="resnet")
    a, b = N.image_pairs(2, 64, 48)
    for net in NETS:
        want = N.forward(net, sds[net], a, b)[0].mean().item()
        got = metrics.LPIPS(a, b, net_type=net)
        assert got.dtype == torch.float32 and got.dim() == 0 and abs(got.item() - want) <= 64 * DEPTH[net] / 5 * U32 * want
        assert torch.equal(got, nets[net](a, b).mean().float()) and metrics.LPIPS(a, a, net_type=net).item() == 0.0
    metrics.configure_lpips(None, net_type="vgg")                        # one type
    assert metrics.lpips_network("vgg") is None and metrics.lpips_network("squeeze") is nets["squeeze"] and metrics.lpips_network("alex") is alex
    metrics.configure_lpips(None)                                        # all three
    assert [metrics.lpips_network(t) for t in ("alex", "vgg", "squeeze")] == [None] * 3
    for net in NETS:
        with pytest.raises(NotImplementedError, match=f"net_type '{net}' is not built in this process"):
            metrics.LPIPS(a, b, net_type=net)
    with pytest.raises(NotImplementedError, match="AlexNet"):
        metrics.LPIPS(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    # by path, by (trunk, lin) pair and by environment variable
    for net in NETS:
        torch.save(sds[net], tmp_path / f"{net}.pth")
        assert isinstance(metrics.configure_lpips(str(tmp_path / f"{net}.pth"), net_type=net), CLASSES[net])
        trunk, lin = N.torchvision_layout(net, sds[net])
        torch.save(trunk, tmp_path / "t.pth")
        torch.save(lin, tmp_path / "l.pth")
        pair = metrics.configure_lpips((tmp_path / "t.pth", tmp_path / "l.pth"), net_type=net)
        assert isinstance(pair, CLASSES[net]) and metrics.lpips_network(net) is pair
    with pytest.raises(KeyError):
        metrics.configure_lpips(str(tmp_path / "vgg.pth"))               # no net_type: 'alex', whose tensors the file does not hold
    metrics.configure_lpips(None)


def test_configure_by_environment(sds, unconfigured, allow_stock, tmp_path, monkeypatch):
    a, b = N.image_pairs(1, 35, 37)
    for net, var in (("vgg", "DMVAE_LPIPS_VGG_WEIGHTS"), ("squeeze", "DMVAE_LPIPS_SQUEEZE_WEIGHTS")):
        torch.save(sds[net], tmp_path / f"{net}.pth")
        monkeypatch.setenv(var, str(tmp_path / f"{net}.pth"))
        want = N.forward(net, sds[net], a, b)[0].mean().item()
        assert abs(metrics.LPIPS(a, b, net_type=net).item() - want) <= 64 * DEPTH[net] / 5 * U32 * want
        assert isinstance(metrics.lpips_network(net), CLASSES[net]) and metrics.lpips_network(net) is metrics.lpips_network(net)      # built once
        assert metrics.lpips_network("alex") is None
        monkeypatch.delenv(var)
        with pytest.raises(NotImplementedError, match="not built"):
            metrics.LPIPS(a, b, net_type=net)


@pytest.mark.parametrize("net", NETS)
def test_stock_composition_matches_the_spec_to_f32_error(sds, nets, allow_stock, net):
    """The stock f32 composition against the f64 specification.  tests/test_lpips_eval_cpu.py argues 64 u for AlexNet's five convolutions: each is a
    blocked f32 sum that adds a relative error of a few u = 2^-24 to a feature vector's L2 norm, the errors of successive layers add (a ReLU, a pool and a
    concat are 1-Lipschitz and exact), and the head forms its normalised differences in f32 from features that carry that error.  The same argument per
    layer gives 64 u x depth / 5 for a trunk whose longest path to a tap has `depth` convolutions: 13 for VGG16 (166 u, 9.9e-6), 17 for SqueezeNet 1.1 --
    features[0] and two convolutions in each of eight Fire modules -- (218 u, 1.3e-5); still four orders below what a wrong tap, a missing bias or a wrong
    channel weight gives.  Measured here: 3e-8 ... 4e-7."""
    forms = ((0, "torchmetrics"), (1, "reference")) if net == "vgg" else ((0, None),)
    for form, normalize in forms:
        m = nets[net]
        if form:
            m = LPIPSVGG(normalize=normalize)
            m.load_state_dict(sds[net])
        for h, w in SIZES[net]:
            a, b = N.image_pairs(3, h, w)
            v64, _, _ = N.forward(net, sds[net], a, b, form=form)
            per = m(a, b)
            assert per.dtype == torch.float64 and tuple(per.shape) == (3,)
            rel = ((per - v64).abs() / v64).max().item()
            print(f"lpips {net} stock f32 route {h} x {w} form {form}: value {v64.mean().item():.6e}, largest relative error {rel:.2e}")
            assert rel <= 64 * DEPTH[net] / 5 * U32
            assert torch.equal(m(a, a), torch.zeros(3, dtype=torch.float64))
            assert torch.equal(m(a.bfloat16(), b.bfloat16()), m(a.bfloat16().float(), b.bfloat16().float()))


@pytest.mark.parametrize("net", NETS)
def test_argument_errors(nets, allow_stock, net):
    m, s = nets[net], CLASSES[net].min_size
    x = torch.zeros(2, 3, 32, 32)
    for bad1, bad2 in ((x + 1.5, x), (x, x - 1.001), (x, x * float("nan"))):
        with pytest.raises(ValueError, match=r"\[-1, 1\]"):
            m(bad1, bad2)
    for bad1, bad2 in ((x[:, :2], x[:, :2]), (x, x[:1]), (x[0], x[0]), (x[:0], x[:0])):
        with pytest.raises(ValueError, match=CLASSES[net].__name__):
            m(bad1, bad2)
    with pytest.raises(ValueError, match=f"at least {s} x {s}"):
        m(torch.zeros(1, 3, s - 1, s), torch.zeros(1, 3, s - 1, s))
    with pytest.raises(ValueError, match=f"at least {s} x {s}"):
        m(torch.zeros(1, 3, s, s - 1), torch.zeros(1, 3, s, s - 1))
    assert m(torch.zeros(1, 3, s, s), torch.zeros(1, 3, s, s)).item() == 0.0


def test_cpu_tensors_need_the_stock_opt_in(nets, monkeypatch):
    from dmvae_amd import _lib
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    x = torch.zeros(1, 3, 32, 32)
    for net in NETS:
        with pytest.raises(_lib.DmvaeHipError, match="DMVAE_ALLOW_STOCK"):
            nets[net](x, x)


# ---- evaluate(..., lpips=net) -----------------------------------------------------------------------------------------------------------------
class StubVAE(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def encode(self, x):
        return x * 0.5

    def decode(self, z):
        return z * 2.6                                                   # leaves [-1, 1]: evaluate clamps what it hands to the metric


@pytest.mark.parametrize("net", NETS)
def test_evaluate_takes_either_network(sds, nets, allow_stock, net):
    from dmvae_amd.evaluate import evaluate
    g = torch.Generator().manual_seed(5)
    imgs = torch.rand(6, 3, 40, 44, generator=g) * 2 - 1
    batches = [(b, torch.zeros(len(b), dtype=torch.long)) for b in imgs.split([1, 3, 2])]
    plain = evaluate(StubVAE(), batches, num_samples=8, device="cpu")
    with_lpips = evaluate(StubVAE(), batches, num_samples=8, device="cpu", lpips=nets[net])
    assert "LPIPS" not in plain and set(with_lpips) == set(plain) | {"LPIPS"} and all(with_lpips[k] == plain[k] for k in plain)
    want = N.forward(net, sds[net], (imgs * 1.3).clamp(-1, 1), imgs)[0].sum().item() / 8
    assert want > 0 and abs(with_lpips["LPIPS"] - want) <= 64 * DEPTH[net] / 5 * U32 * want


# ---- the launcher -----------------------------------------------------------------------------------------------------------------------------
def test_launcher_flags_imply_hip_metrics_and_configure_each_type(sds, tmp_path):
    for net in NETS:
        torch.save(sds[net], tmp_path / f"{net}.pth")
    env = {k: v for k, v in os.environ.items() if k not in ("DMVAE_HIP_METRICS",) + ENV}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_on_mi355x.py"), f"--lpips-vgg-weights={tmp_path / 'vgg.pth'}",
                        f"--lpips-squeeze-weights={tmp_path / 'squeeze.pth'}", "--check"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "evaluation.metrics" in r.stdout and "dmvae_amd.metrics" in r.stdout                      # the flags imply --hip-metrics
    assert "net_type='vgg'" in r.stdout and "LPIPSVGG" in r.stdout and "net_type='squeeze'" in r.stdout and "LPIPSSqueeze" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_on_mi355x.py"), "--check"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "evaluation.metrics" not in r.stdout and "LPIPSVGG" not in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_on_mi355x.py"), f"--lpips-vgg-weights={tmp_path / 'squeeze.pth'}", "--check"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "KeyError" in r.stderr                                              # the wrong file for the type says so
