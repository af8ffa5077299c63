"""bench.py's plain run measures the headline only; `--full` adds the measurements that take runs of their own (kl_mmd, comm_n1, the c3 / c4 / gan
stages, cpu_baseline), and its --no-secondary / --no-cpu-baseline switches leave parts of that out."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"kl_mmd", "comm_n1", "c3_dmd_cycle", "c4_diffusion_step", "gan_step", "secondary_error", "cpu_baseline"}
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config", "env",
            "ms_per_step_windows", "roofline", "roofline_wgrad", "linear_gemm"}


def _line(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *args],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])


def test_bench_has_a_full_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout


@pytest.mark.gpu
def test_plain_run_carries_the_headline_only_and_full_adds_the_rest():
    plain = _line()
    assert HEADLINE <= set(plain) and not FULL_ONLY & set(plain), sorted(plain)
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["roofline"]["launches"] > 0
    full = _line("--full", "--no-secondary", "--no-cpu-baseline")
    assert HEADLINE <= set(full) and FULL_ONLY & set(full) == {"kl_mmd"}, sorted(full)
    assert all(full["kl_mmd"][k]["us_per_call"] > 0 for k in ("fused_B32", "kl_pass_268MB", "fused_B1024"))
