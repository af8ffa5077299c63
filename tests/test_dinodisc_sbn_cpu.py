"""CPU: DinoDisc with SyncBatchNorm heads -- the configuration the reference's trainers build (norm_type "sbn", use_specnorm False; train_tokenizer.py:48-49,
307-314) -- against captures from the reference's own module (tools/capture_golden_dinodisc_sbn.py -> tests/golden/dinodisc_sbn_{small,manifest}.npz): the f32
twin tests/dinodisc_sbn_spec.py, which states the norm by its formulas, and the module's `forward_stock`, at the bars tests/test_dinodisc_cpu.py holds the same
quantities to -- rel_err 2e-5 on logits, 1e-4 on gradients and gradient norms, 1e-7 of the weight-gradient norm for the conv biases in front of a train-mode norm
(analytically zero) -- plus 2e-5 on the running statistics after each of two calls and the counter exactly; the switch in front of the variants; and, over two
gloo processes with unequal batches (8 and 4), the statistics combination the head calls and the twin with explicit cross-rank sums against the union batch."""
import os
import random
import socket
import subprocess
import sys

import pytest
import torch

import dinodisc_spec as S
import dinodisc_sbn_spec as SB
from conftest import ROOT, load_golden, rel_err

ZERO_GRAD_FACTOR = 1e-7                  # tests/test_dinodisc_cpu.py
STATE = ("running_mean", "running_var", "num_batches_tracked")


@pytest.fixture
def area_branch(monkeypatch):
    monkeypatch.setattr(random, "random", lambda: 0.75)


@pytest.fixture
def syncbn_on(monkeypatch):
    import dmvae_amd.models.dinodisc as D
    monkeypatch.setattr(D, "_SYNCBN_HEADS", True)


def check_head_grads(g, grads):
    for k, gr in grads.items():
        if k.endswith(".0.bias"):            # heads.i.0.0.bias, heads.i.1.fn.0.bias: in front of a norm with batch statistics
            assert gr.abs().max().item() <= ZERO_GRAD_FACTOR * float(g["gn." + k[:-4] + "weight"]), k
        elif "g." + k in g:
            assert rel_err(gr, g.t("g." + k)) < 1e-4, k
        else:
            stride = 97 if gr.numel() < 200000 else 997
            assert rel_err(gr.flatten()[::stride], g.t("gs." + k)) < 1e-4, k
            assert abs(gr.double().norm().item() - float(g["gn." + k])) < 1e-4 * float(g["gn." + k]), k
            assert abs(gr.double().sum().item() - float(g["gsum." + k])) < 1e-4 * float(g["gn." + k]), k


def check_state(g, tag, state):
    seen = 0
    for k, v in state.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(g[tag + k]), k
        elif k.endswith(STATE):
            assert rel_err(v, g.t(tag + k)) < 2e-5, (tag, k)
        else:
            continue
        seen += 1
    assert seen == 3 * 2 * len(SB.SMALL["key_depths"])


def test_spec_twin_in_f32_vs_reference(syncbn_on):
    g, c = load_golden("dinodisc_sbn_small"), SB.SMALL
    _, backbone, heads = SB.build_module()
    x, x2 = S.image(c["batch"], c["px"], c["x_seed"]), S.image(c["batch"], c["px"], c["x_seed"] + 1)
    p = {k: v.clone().requires_grad_(SB.is_param(k)) for k, v in heads.items()}
    st1 = {}
    logits = SB.forward(x, backbone, p, train=True, new_state=st1)
    assert logits.shape == (12, 648) and rel_err(logits.detach(), g.t("logits_train")) < 2e-5
    dy = torch.randn(logits.shape, generator=torch.Generator().manual_seed(c["dy_seed"]))
    (logits * dy).sum().backward()
    check_head_grads(g, {k: v.grad for k, v in p.items() if v.requires_grad})
    check_state(g, "st1.", st1)
    st2 = {}
    with torch.no_grad():
        l2 = SB.forward(x2, backbone, {**heads, **st1}, train=True, new_state=st2)
    assert rel_err(l2, g.t("logits_train2")) < 2e-5
    check_state(g, "st2.", st2)
    xe = x.clone().requires_grad_(True)
    le = SB.forward(xe, backbone, heads, train=False)
    assert rel_err(le.detach(), g.t("logits_eval")) < 2e-5
    (le * dy).sum().backward()
    assert rel_err(xe.grad[:, :, ::16, ::16], g.t("dx_slice")) < 1e-4
    assert abs(xe.grad.double().norm().item() - float(g["dx_norm"])) < 1e-4 * float(g["dx_norm"])


def test_state_dict_keys_and_strict_load(syncbn_on):
    import warnings
    from dmvae_amd.models.dinodisc import DinoDisc
    m = load_golden("dinodisc_sbn_manifest")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        disc = DinoDisc(9, "cpu", None, key_depths=(0, 2, 5, 8, 11), norm_type="sbn", norm_eps=1e-6, use_specnorm=False)
    sd = disc.state_dict()
    keys = [str(k) for k in m["disc_keys"]]
    assert list(sd.keys()) == keys and len(keys) == 2 + 5 * 16
    shapes = {}
    for k, s in zip(keys, m["disc_shapes"]):
        shapes[k] = tuple(int(d) for d in s if d >= 0)
        assert tuple(sd[k].shape) == shapes[k], k
    assert {"heads.4.0.1.running_var", "heads.0.1.fn.1.num_batches_tracked", "heads.2.0.0.weight", "heads.3.2.bias"} <= set(keys)
    ref_sd = SB.filled_heads(shapes, 5)                       # a reference-format state_dict: the manifest's keys and shapes
    ref_sd.update(x_scale=sd["x_scale"].clone(), x_shift=sd["x_shift"].clone())
    disc.load_state_dict(ref_sd, strict=True)
    got = disc.state_dict()
    assert all(torch.equal(got[k], ref_sd[k]) for k in keys)
    assert got["heads.0.0.1.num_batches_tracked"].dtype == torch.int64 and (got["heads.1.0.1.running_var"] > 0).all()
    for nt in ("lbn", "hbn"):                                  # no process group in a single process: the same module
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            d2 = DinoDisc(9, "cpu", None, key_depths=(0,), dino_depth=1, norm_type=nt, use_specnorm=False)
        assert isinstance(d2.heads[0][0][1], torch.nn.SyncBatchNorm) and d2.heads[0][0][1].process_group is None


def test_stock_route_vs_reference(syncbn_on, area_branch):
    g, c = load_golden("dinodisc_sbn_small"), SB.SMALL
    disc, _, heads = SB.build_module()
    x, x2 = S.image(c["batch"], c["px"], c["x_seed"]), S.image(c["batch"], c["px"], c["x_seed"] + 1)
    disc.train()
    logits = disc.forward_stock(x)
    assert logits.shape == (12, 648) and rel_err(logits.detach(), g.t("logits_train")) < 2e-5
    dy = torch.randn(logits.shape, generator=torch.Generator().manual_seed(c["dy_seed"]))
    (logits * dy).sum().backward()
    check_head_grads(g, {k: p.grad for k, p in disc.named_parameters()})
    check_state(g, "st1.", disc.state_dict())
    with torch.no_grad():
        assert rel_err(disc.forward_stock(x2), g.t("logits_train2")) < 2e-5
    check_state(g, "st2.", disc.state_dict())
    disc.load_state_dict(heads, strict=False)
    disc.eval().requires_grad_(False)
    xe = x.clone().requires_grad_(True)
    le = disc.forward_stock(xe)
    assert rel_err(le.detach(), g.t("logits_eval")) < 2e-5
    (le * dy).sum().backward()
    assert rel_err(xe.grad[:, :, ::16, ::16], g.t("dx_slice")) < 1e-4
    assert abs(xe.grad.double().norm().item() - float(g["dx_norm"])) < 1e-4 * float(g["dx_norm"])
    sd = disc.state_dict()
    assert all(torch.equal(sd[k], heads[k]) for k in sd if k.endswith(STATE))       # eval: the estimates are constants


def test_switch_is_off_by_default_and_names_how_to_turn_it_on(monkeypatch):
    import warnings
    import dmvae_amd.models.dinodisc as D
    assert D._SYNCBN_HEADS is False
    for nt in ("sbn", "lbn", "hbn"):
        with pytest.raises(NotImplementedError, match=r"dinodisc.py:62-65.*enable_syncbn_heads"):
            D.DinoDisc(9, "cpu", None, norm_type=nt, dino_depth=1, key_depths=(0,))
    monkeypatch.setattr(D, "_SYNCBN_HEADS", False)            # restored whatever the calls below leave
    assert D.enable_syncbn_heads() is False and D._SYNCBN_HEADS is True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        disc = D.DinoDisc(9, "cpu", None, norm_type="sbn", use_specnorm=False, dino_depth=1, key_depths=(0,))
    n = disc.heads[0][1].fn[1]
    assert isinstance(n, torch.nn.SyncBatchNorm) and n.eps == 1e-6 and n.momentum == 0.1 and n.process_group is None
    assert D.enable_syncbn_heads(False) is True and D._SYNCBN_HEADS is False


def test_shadow_turns_the_switch_on_only_with_the_opt_in():
    code = r"""
import sys, os, tempfile
sys.path.insert(0, %r)
import run_on_mi355x as L
ref = tempfile.mkdtemp()
os.makedirs(os.path.join(ref, "models"))
open(os.path.join(ref, "models", "dinodisc.py"), "w").write("class DinoDisc: marker = 'reference file'\n")
optin = sys.argv[1] == "1"
L.install_shadow(ref, dinodisc=True) if optin else L.install_shadow(ref)
import dmvae_amd.models.dinodisc as ours
assert ours._SYNCBN_HEADS is optin
if optin:
    import warnings
    from models import DinoDisc
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d = DinoDisc(device="cpu", ks=9, dino_ckpt=None, key_depths=(0,), norm_type="sbn", norm_eps=1e-6, use_specnorm=False, dino_depth=1)
    assert "heads.0.0.1.running_mean" in d.state_dict()
print("switch ok")
""" % ROOT
    for optin in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code, optin], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "switch ok" in r.stdout, r.stderr[-2000:]


# ---- two gloo processes, batches of 8 and 4 -------------------------------------------------------------------------------------------------------------------
GLOO = dict(depth=2, key_depths=(0, 1), ks=9, px=70, seed=41, shares=(8, 4))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gloo_worker(rank, world, port, q):
    torch.cuda.is_available = lambda: False
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as tdist
    import torch.distributed.nn.functional as dfn
    import dmvae_amd.models.dinodisc as D
    from dmvae_amd import dist
    from dmvae_amd.models.patchgan import sync_batch_stats
    dist.init_distributed_mode(backend="gloo")
    c = GLOO
    lo, hi = sum(c["shares"][:rank]), sum(c["shares"][:rank + 1])
    ok = {}
    # (1) the helper the head's statistics pass through (models.patchgan._bn_stats -> sync_batch_stats): the union's mean, biased variance and count
    full = torch.randn(12, 25, 16, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 1.5 + 0.7
    mine = full[lo:hi].reshape(-1, 16)
    mean, var, n = sync_batch_stats(mine.mean(0), mine.var(0, unbiased=False), mine.shape[0])
    allr = full.reshape(-1, 16)
    ok["count"] = n == 12 * 25
    ok["mean"] = rel_err(mean, allr.mean(0)) < 1e-12
    ok["var"] = rel_err(var, allr.var(0, unbiased=False)) < 1e-12
    # (2) the twin with explicit cross-rank sums against the twin on the concatenated batch, f64
    D.enable_syncbn_heads()
    _, backbone, heads = SB.build_module(depth=c["depth"], key_depths=c["key_depths"], ks=c["ks"], seed=c["seed"])
    dbl = lambda d: {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in d.items()}
    backbone, heads = dbl(backbone), dbl(heads)
    x = S.image(12, c["px"], 3).double()
    dy = torch.randn(12, 2 * 25, generator=torch.Generator().manual_seed(4), dtype=torch.float64)

    def run(xs, dys, reduce):
        p = {k: v.clone().requires_grad_(SB.is_param(k)) for k, v in heads.items()}
        st = {}
        logits = SB.forward(xs, backbone, p, ks=c["ks"], key_depths=c["key_depths"], train=True, branch="bicubic", new_state=st, reduce=reduce)
        (logits * dys).sum().backward()
        return logits.detach(), {k: v.grad for k, v in p.items() if v.requires_grad}, st

    l_all, g_all, st_all = run(x, dy, None)
    l_mine, g_mine, st_mine = run(x[lo:hi], dy[lo:hi], lambda v: dfn.all_reduce(v))
    ok["logits"] = rel_err(l_mine, l_all[lo:hi]) < 1e-10
    for k, gr in g_mine.items():
        gr = gr.clone()
        tdist.all_reduce(gr)
        scale = max(g_all[k].abs().max().item(), 1e-6 * max(v.abs().max().item() for v in g_all.values()))      # (the zero-gradient biases: an absolute bar)
        ok["grad " + k] = (gr - g_all[k]).abs().max().item() < 1e-9 * scale
    for k, v in st_all.items():
        ok["state " + k] = (int(v) == int(st_mine[k])) if k.endswith("num_batches_tracked") else rel_err(st_mine[k], v) < 1e-12
    dist.barrier()
    q.put((rank, sorted(k for k, v in ok.items() if not v)))
    tdist.destroy_process_group()


def test_two_gloo_ranks_with_unequal_batches():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    got = sorted(q.get(timeout=5) for _ in range(2))
    assert got == [(0, []), (1, [])], got


def test_new_local_machine_group_without_a_process_group():
    from dmvae_amd import dist
    assert dist.new_local_machine_group() is None
