"""CPU: the two entry points of csrc/ssim.hip are exported and bound, the workspace size is its closed form, and dmvae_ssim validates its arguments before
any HIP call -- -22 plus a message that carries the entry's name, no GPU touched.  The entries are additive: the ABI version does not move."""
import ctypes
import math
import os
import subprocess

import pytest

from conftest import ROOT

ENTRIES = {"dmvae_ssim_workspace": 4, "dmvae_ssim": 12}


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_ssim_entries_are_exported_and_bound(lib):
    from dmvae_amd import _lib
    for name, nargs in ENTRIES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["dmvae_ssim"][1][8] is ctypes.c_double                # data_range
    assert lib.dmvae_abi_version() == 9 and _lib.ABI_VERSION == 9
    with open(os.path.join(ROOT, "include", "dmvae_hip.h")) as fh:
        header = fh.read()
    assert "size_t dmvae_ssim_workspace(size_t batch, int channels, int h, int w);" in header and "int dmvae_ssim(const void* a, const void* b," in header


def test_workspace_is_one_f64_per_plane_and_tile(lib):
    ws = lib.dmvae_ssim_workspace
    for b, c, h, w in ((1, 1, 11, 11), (3, 2, 11, 75), (1, 1, 26, 42), (1, 1, 27, 43), (2, 3, 37, 53), (5, 3, 64, 64), (2, 3, 256, 256), (32, 3, 256, 256)):
        assert ws(b, c, h, w) == b * c * math.ceil((w - 10) / 32) * math.ceil((h - 10) / 16) * 8, (b, c, h, w)
    assert ws(1, 1, 26, 42) == 8 and ws(1, 1, 27, 43) == 32 and ws(2, 3, 256, 256) == 2 * 3 * 128 * 8
    assert ws(2, 3, 10, 64) == 0 and ws(2, 3, 64, 10) == 0 and ws(2, 0, 64, 64) == 0 and ws(0, 3, 64, 64) == 0


def test_ssim_rejects_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.dmvae_ssim

    def rejected(*args):
        rc = f(*args)
        msg = lib.dmvae_last_error()
        assert rc == -22 and b"ssim" in msg, (rc, msg)
        return msg
    #   a, b, is_bf16, batch, channels, h, w, from_pm1, data_range, workspace, out, stream
    for i in (0, 1, 9, 10):                                                       # each null pointer
        a = [p, p, 0, 2, 3, 64, 64, 0, 1.0, p, p]
        a[i] = None
        assert b"NULL" in rejected(*a, None)
    assert b"h >= 11" in rejected(p, p, 0, 2, 3, 10, 64, 0, 1.0, p, p, None)
    assert b"w >= 11" in rejected(p, p, 1, 2, 3, 64, 10, 1, 1.0, p, p, None)
    assert b"h >= 11" in rejected(p, p, 0, 2, 3, -5, 64, 0, 1.0, p, p, None)
    assert b"channels" in rejected(p, p, 0, 2, 0, 64, 64, 0, 1.0, p, p, None)
    assert b"channels" in rejected(p, p, 0, 2, -3, 64, 64, 0, 1.0, p, p, None)
    assert b"batch" in rejected(p, p, 0, 0, 3, 64, 64, 0, 1.0, p, p, None)
    for dr in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert b"data_range" in rejected(p, p, 0, 2, 3, 64, 64, 0, dr, p, p, None)
    # planes x tiles lie flat on grid.x: beyond 2^31 - 1 blocks the call is refused, not wrapped
    assert b"2^31" in rejected(p, p, 0, 1 << 24, 3, 256, 256, 0, 1.0, p, p, None)
    assert lib.dmvae_abi_version() == 9


def test_ops_ssim_refuses_cpu_tensors():
    import torch
    from dmvae_amd import _lib, ops
    with pytest.raises(_lib.DmvaeHipError):
        ops.ssim(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
