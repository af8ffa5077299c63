"""CPU: the multi-tensor optimiser tail (csrc/optim_mt.hip; the reference's own loop, train_tokenizer.py:140-150,382,415-419) is declared, exported and bound; its
entry points validate their arguments before any HIP call; `optim.AdamW` keeps torch.optim.AdamW's state layout, refuses to fall back silently and, opted in to the
stock route, IS the parent; the launcher's --hip-optim replaces the two attributes of torch and nothing else does."""
import copy
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

MT = ("dmvae_mt_chunk_elems", "dmvae_mt_grad_norm_workspace", "dmvae_mt_grad_norm", "dmvae_mt_scale_grads", "dmvae_mt_adamw_ema_step", "dmvae_mt_ema")


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_mt_entries_are_declared_exported_and_bound(lib):
    from dmvae_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    for name in MT:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert decl, f"{name} is not declared in include/dmvae_hip.h"
        n_args = 0 if decl.group(1).strip() in ("", "void") else decl.group(1).count(",") + 1
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name)
    assert lib.dmvae_abi_version() == 9                   # a compatible extension: the version does not move
    c = lib.dmvae_mt_chunk_elems()
    assert c >= 1024 and c % 4 == 0
    assert lib.dmvae_mt_grad_norm_workspace(10) >= 40
    # the structs the tables are built as: six and two 8-byte words
    assert re.search(r"typedef struct dmvae_mt_tensor \{\s*void\* p;\s*void\* g;\s*void\* m;\s*void\* v;\s*void\* ema;\s*size_t numel;\s*\}", hdr)
    assert re.search(r"typedef struct dmvae_mt_chunk \{\s*size_t tensor;\s*size_t first;\s*\}", hdr)


def test_mt_entries_reject_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def rejected(rc, *words):
        msg = lib.dmvae_last_error()
        assert rc == -22 and all(w in msg for w in words), (rc, msg)

    hyper = (1e-4, 0.9, 0.95, 1e-8, 0.005)
    # null table / null chunk list, every entry
    rejected(lib.dmvae_mt_grad_norm(None, 1, p, 1, p, p, 4096, 1.0, None), b"mt_grad_norm", b"null table")
    rejected(lib.dmvae_mt_grad_norm(p, 1, None, 1, p, p, 4096, 1.0, None), b"mt_grad_norm", b"null chunk list")
    rejected(lib.dmvae_mt_scale_grads(None, 1, p, 1, p, None), b"mt_scale_grads", b"null table")
    rejected(lib.dmvae_mt_scale_grads(p, 1, None, 1, p, None), b"mt_scale_grads", b"null chunk list")
    rejected(lib.dmvae_mt_adamw_ema_step(None, 1, p, 1, None, *hyper, 1, 0.9999, None), b"mt_adamw_ema_step", b"null table")
    rejected(lib.dmvae_mt_adamw_ema_step(p, 1, None, 1, None, *hyper, 1, 0.9999, None), b"mt_adamw_ema_step", b"null chunk list")
    rejected(lib.dmvae_mt_ema(None, 1, p, 1, 0.9999, None), b"mt_ema", b"null table")
    rejected(lib.dmvae_mt_ema(p, 1, None, 1, 0.9999, None), b"mt_ema", b"null chunk list")
    # workspace too small: one f32 per chunk
    rejected(lib.dmvae_mt_grad_norm(p, 1, p, 100, p, p, 399, 1.0, None), b"mt_grad_norm", b"workspace too small")
    rejected(lib.dmvae_mt_grad_norm(p, 1, p, 1, p, None, 4096, 1.0, None), b"mt_grad_norm", b"null")
    rejected(lib.dmvae_mt_scale_grads(p, 1, p, 1, None, None), b"mt_scale_grads", b"null")
    # step counts from 1
    rejected(lib.dmvae_mt_adamw_ema_step(p, 1, p, 1, None, *hyper, 0, 0.9999, None), b"mt_adamw_ema_step", b"step")
    rejected(lib.dmvae_mt_adamw_ema_step(p, 1, p, 1, None, *hyper, -3, 0.9999, None), b"mt_adamw_ema_step", b"step")
    # an empty table: 0, nothing launched (no GPU here: a launch would return -5)
    assert lib.dmvae_mt_grad_norm(None, 0, None, 0, p, p, 4096, 1.0, None) == 0
    assert lib.dmvae_mt_scale_grads(None, 0, None, 0, p, None) == 0
    assert lib.dmvae_mt_adamw_ema_step(None, 0, None, 0, None, *hyper, 1, 0.9999, None) == 0
    assert lib.dmvae_mt_ema(None, 0, None, 0, 0.9999, None) == 0
    assert lib.dmvae_abi_version() == 9


def _twins(seed=0):
    torch.manual_seed(seed)
    a = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(2, 2, 2))]
    b = [torch.nn.Parameter(x.detach().clone()) for x in a]
    return a, b


def _feed(a, b, seed):
    gen = torch.Generator().manual_seed(seed)
    for x, y in zip(a, b):
        g = torch.randn(x.shape, generator=gen)
        x.grad, y.grad = g.clone(), g.clone()


KW = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.005)


def test_adamw_on_cpu_parameters_does_not_fall_back_silently(monkeypatch):
    from dmvae_amd import optim
    from dmvae_amd._lib import DmvaeHipError
    monkeypatch.delenv("DMVAE_ALLOW_STOCK", raising=False)
    a, b = _twins()
    opt = optim.AdamW(a, **KW)
    _feed(a, b, 1)
    with pytest.raises(DmvaeHipError, match="optim.AdamW.step"):
        opt.step()
    with pytest.raises(DmvaeHipError, match="optim.clip_grad_norm_"):
        optim.clip_grad_norm_(a, 1.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not opt.state       # nothing moved, no state was made


def test_adamw_opted_in_to_the_stock_route_is_the_parent_bit_for_bit(allow_stock):
    from dmvae_amd import optim
    a, b = _twins()
    ours, stock = optim.AdamW(a, **KW), torch.optim.AdamW(b, **KW)
    lam = lambda s: min(1.0, s / 2)                                               # the first step runs at lr 0 (train_tokenizer.py:385-392)
    sched_a, sched_b = torch.optim.lr_scheduler.LambdaLR(ours, lam), torch.optim.lr_scheduler.LambdaLR(stock, lam)
    lrs = []
    for it in range(3):
        _feed(a, b, 10 + it)
        na, nb = optim.clip_grad_norm_(a, 1.0), torch.nn.utils.clip_grad_norm_(b, 1.0)
        assert torch.equal(na, nb) and all(torch.equal(x.grad, y.grad) for x, y in zip(a, b))
        lrs.append(ours.param_groups[0]["lr"])
        ours.step()
        stock.step()
        ours.zero_grad(set_to_none=True)
        stock.zero_grad(set_to_none=True)
        sched_a.step()
        sched_b.step()
        assert all(torch.equal(x, y) for x, y in zip(a, b)), it
    assert lrs == [0.0, 0.005, 0.01]                                              # LambdaLR drives it: group["lr"] is read at step time
    m = torch.nn.Linear(3, 2)
    e = torch.nn.Linear(3, 2)
    e.load_state_dict(m.state_dict())
    with torch.no_grad():
        m.weight.add_(1.0)
    want = e.weight.detach() * 0.9 + m.weight.detach() * (1 - 0.9)
    optim.update_ema(e, m, decay=0.9)                                            # the scripts' signature, on the stock route here
    assert torch.allclose(e.weight, want, rtol=1e-6)


def test_state_dict_has_the_parents_layout_and_loads_both_ways(allow_stock):
    from dmvae_amd import optim
    a, b = _twins()
    ours, stock = optim.AdamW(a, **KW), torch.optim.AdamW(b, **KW)
    for it in range(2):
        _feed(a, b, 20 + it)
        ours.step()
        stock.step()
    sd, ref = ours.state_dict(), stock.state_dict()
    assert sd.keys() == ref.keys() and sd["param_groups"][0].keys() == ref["param_groups"][0].keys()
    assert sd["param_groups"][0] == ref["param_groups"][0]
    assert sd["state"].keys() == ref["state"].keys()
    for i in sd["state"]:
        assert list(sd["state"][i]) == ["step", "exp_avg", "exp_avg_sq"] == list(ref["state"][i])
        for k in sd["state"][i]:
            x, y = sd["state"][i][k], ref["state"][i][k]
            assert type(x) is type(y) and x.dtype == y.dtype and x.device == y.device and x.shape == y.shape and torch.equal(x, y), (i, k)
    # ours -> a fresh torch.optim.AdamW, torch's -> a fresh one of ours; then one more step on all four
    c, d = _twins()
    with torch.no_grad():
        for x, y, z in zip(c, d, a):
            x.copy_(z)
            y.copy_(z)
    fresh_stock, fresh_ours = torch.optim.AdamW(c, **KW), optim.AdamW(d, **KW)
    fresh_stock.load_state_dict(copy.deepcopy(sd))          # (load_state_dict keeps tensors that need no cast: without the copy the twins would share state)
    fresh_ours.load_state_dict(copy.deepcopy(ref))
    _feed(a, b, 30)
    _feed(c, d, 30)
    for o in (ours, stock, fresh_stock, fresh_ours):
        o.step()
    for x, y, z, w in zip(a, b, c, d):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, w)
    assert float(fresh_ours.state[d[0]]["step"]) == 3.0


def test_a_flat_buffer_owned_parameter_is_refused():
    from dmvae_amd import optim
    a, _ = _twins()
    optim.FlatParams(a, with_ema=False)
    with pytest.raises(ValueError, match="FlatParams"):
        optim.AdamW(a, **KW)
    c, _ = _twins()
    opt = optim.AdamW(c, **KW)               # re-homed after construction: refused at the step
    optim.FlatParams(c, with_ema=False)
    with pytest.raises(ValueError, match="FlatParams"):
        opt.step()


def test_attach_ema_takes_only_this_optimisers_pairs():
    from dmvae_amd import optim
    a, b = _twins()
    opt = optim.AdamW(a, **KW)
    with pytest.raises(ValueError, match="attach_ema"):
        opt.attach_ema([(torch.zeros(5, 3), b[0])])


def test_launcher_replaces_the_two_torch_attributes_only_when_asked():
    code = r"""
import sys
sys.path.insert(0, %r)
import torch
adamw, clip = torch.optim.AdamW, torch.nn.utils.clip_grad_norm_
import run_on_mi355x as L
import dmvae_amd.optim as ours
assert torch.optim.AdamW is adamw and torch.nn.utils.clip_grad_norm_ is clip             # importing touches nothing
if sys.argv[1] == "1":
    L.install_shadow(None, optim=True)
    assert torch.optim.AdamW is ours.AdamW and torch.nn.utils.clip_grad_norm_ is ours.clip_grad_norm_
    assert issubclass(torch.optim.AdamW, adamw) and ours._TORCH_CLIP is clip
else:
    L.install_shadow(None)
    assert torch.optim.AdamW is adamw and torch.nn.utils.clip_grad_norm_ is clip
print("optim ok")
""" % ROOT
    env = {k: v for k, v in os.environ.items() if k != "DMVAE_HIP_OPTIM"}
    for optin in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code, optin], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and "optim ok" in r.stdout, r.stderr[-2000:]
    launcher = os.path.join(ROOT, "run_on_mi355x.py")
    for argv, e in ((["--hip-optim", "--check"], env), (["--hip-dinodisc", "--hip-optim", "--check"], env), (["--hip-optim", "--hip-dinodisc", "--check"], env),
                    (["--check"], dict(env, DMVAE_HIP_OPTIM="1"))):
        r = subprocess.run([sys.executable, launcher] + argv, capture_output=True, text=True, timeout=300, env=e)
        assert r.returncode == 0, r.stderr[-2000:]
        assert re.search(r"torch\.optim\.AdamW\s+-> dmvae_amd\.optim\.AdamW", r.stdout), r.stdout
        assert re.search(r"torch\.nn\.utils\.clip_grad_norm_\s+-> dmvae_amd\.optim\.clip_grad_norm_", r.stdout), r.stdout
        assert ("dmvae_amd.models.dinodisc" in r.stdout) == ("--hip-dinodisc" in argv)
    r = subprocess.run([sys.executable, launcher, "--check"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "torch." not in r.stdout, r.stderr[-2000:]
