"""bench.py --dump-outputs DIR: what the last timed step returned, as float32 .npy files within 64 MB, the same positions on every run; and --steps is the
number of timed steps.  The helper is exercised on the CPU with a stand-in trainer; the real command runs on the GPU box."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    # bench.py fills in this variable at import when it is unset: keep the test process's environment as it was
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import bench as b
    return b


def _fake_trainer(n, seed):
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(n, generator=g)
    fp = types.SimpleNamespace(flat=flat, ema=flat * 0.5, grad=torch.randn(n, generator=g))
    return types.SimpleNamespace(fp=fp, log=torch.arange(8, dtype=torch.float32))


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_small_buffer_is_written_whole(bench, tmp_path):
    tr = _fake_trainer(1000, 0)
    bench.dump_outputs(str(tmp_path), tr, torch.tensor(1.25))
    got = _read(tmp_path)
    assert set(got) == {"loss", "log", "params", "ema", "grad"}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].shape == () and got["loss"] == np.float32(1.25)
    assert np.array_equal(got["log"], np.arange(8, dtype=np.float32))
    assert np.array_equal(got["params"], tr.fp.flat.numpy()) and np.array_equal(got["ema"], tr.fp.ema.numpy())
    assert np.array_equal(got["grad"], tr.fp.grad.numpy())


def test_dump_large_buffer_is_a_fixed_sample_within_budget(bench, tmp_path):
    n = 6_000_000                                             # 72 MB per flat array: over the budget on its own
    tr = _fake_trainer(n, 1)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), tr, torch.tensor(0.5))
    bench.dump_outputs(str(b), _fake_trainer(n, 1), torch.tensor(0.5))
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert total <= 64 << 20, total
    ga, gb = _read(a), _read(b)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k                # same inputs, same positions
    assert 0 < ga["params"].size < n and ga["params"].size == ga["ema"].size == ga["grad"].size
    assert np.array_equal(ga["ema"], ga["params"] * np.float32(0.5))      # every flat array is sampled at the same positions
    assert np.isin(ga["params"][:100], tr.fp.flat.numpy()).all()


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr and '"metric"' not in r.stdout


@pytest.mark.gpu
def test_bench_dump_outputs_of_the_timed_steps(tmp_path):
    """The real command: --steps sets the timed steps of the line, and the dump holds the last step's finite outputs with the loss the line reports."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-secondary",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
    assert d["steps"] == 2 and d["warmup"] == 1
    got = _read(tmp_path)
    assert set(got) == {"loss", "log", "params", "ema", "grad"}
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 << 20
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert abs(float(got["log"][3]) - d["config"]["loss_after_run"]) < 1e-4 * max(1.0, abs(d["config"]["loss_after_run"]))
    assert np.abs(got["grad"]).max() > 0
