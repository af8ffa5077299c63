"""CPU: the three entry points of csrc/fidelity.hip are exported and bound, the Inception Score's workspace size is its closed form, and both kernels'
entries validate their arguments before any HIP call -- -22 plus a message that carries the entry's name, no GPU touched.  The entries are additive: the ABI
version does not move."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

ENTRIES = {"dmvae_resize_tf1_bilinear": 9, "dmvae_inception_score_workspace": 3, "dmvae_inception_score": 10}


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_fidelity_entries_are_exported_and_bound(lib):
    from dmvae_amd import _lib
    for name, nargs in ENTRIES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["dmvae_inception_score_workspace"][0] is ctypes.c_size_t
    assert lib.dmvae_abi_version() == 9 and _lib.ABI_VERSION == 9
    with open(os.path.join(ROOT, "include", "dmvae_hip.h")) as fh:
        header = fh.read()
    assert "int dmvae_resize_tf1_bilinear(const uint8_t* img, size_t batch, int channels, int h, int w, int nhwc, int s, float* out," in header
    assert "size_t dmvae_inception_score_workspace(size_t n, int classes, size_t splits);" in header
    assert "int dmvae_inception_score(const void* logits, int dtype, size_t n, int classes, size_t ld, const int64_t* order, size_t splits," in header
    for ref in ("sample_50k.py:174-209", "evaluation/fid.py:8-48"):
        assert header.count(ref) >= 3, ref


def test_workspace_is_two_f64_per_row_and_one_per_split_and_class(lib):
    ws = lib.dmvae_inception_score_workspace
    for n, c, s in ((1, 2, 1), (10, 8, 10), (23, 1008, 10), (257, 1008, 10), (50000, 1008, 10), (37, 5, 1), (70000, 65536, 3), ((1 << 31) - 1, 1000, 10)):
        assert ws(n, c, s) == (2 * n + s * c) * 8, (n, c, s)
    assert ws(50000, 1008, 10) == 880640
    # 0 where the kernel's entry refuses: classes outside [2, 65536], splits outside [1, n], n beyond 2^31 - 1
    assert ws(10, 1, 2) == 0 and ws(10, 65537, 2) == 0 and ws(10, -8, 2) == 0
    assert ws(10, 8, 0) == 0 and ws(10, 8, 11) == 0 and ws(0, 8, 1) == 0 and ws(1 << 31, 8, 10) == 0


def test_resize_rejects_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.dmvae_resize_tf1_bilinear

    def rejected(*args):
        rc = f(*args)
        msg = lib.dmvae_last_error()
        assert rc == -22 and b"resize_tf1_bilinear" in msg, (rc, msg)
        return msg
    #   img, batch, channels, h, w, nhwc, s, out, stream
    assert b"NULL" in rejected(None, 2, 3, 16, 16, 1, 8, p, None)
    assert b"NULL" in rejected(p, 2, 3, 16, 16, 1, 8, None, None)
    assert b"batch" in rejected(p, 0, 3, 16, 16, 1, 8, p, None)
    assert b"channels" in rejected(p, 2, 0, 16, 16, 0, 8, p, None)
    assert b"channels" in rejected(p, 2, -3, 16, 16, 0, 8, p, None)
    assert b"h >= 1" in rejected(p, 2, 3, 0, 16, 1, 8, p, None)
    assert b"w >= 1" in rejected(p, 2, 3, 16, -1, 1, 8, p, None)
    assert b"s >= 1" in rejected(p, 2, 3, 16, 16, 1, 0, p, None)
    assert b"s >= 1" in rejected(p, 2, 3, 16, 16, 0, -299, p, None)
    # outputs lie flat on grid.x: beyond (2^31 - 1) * 256 of them the call is refused, not wrapped
    assert b"2^31" in rejected(p, 1 << 24, 3, 16, 16, 1, 299, p, None)
    assert b"2^31" in rejected(p, 1, 3, 16, 16, 1, 1 << 20, p, None)
    assert b"2^31" in rejected(p, 1, (1 << 31) - 1, 16, 16, 1, (1 << 31) - 1, p, None)      # the product wraps 64 bits
    assert lib.dmvae_abi_version() == 9


def test_inception_score_rejects_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.dmvae_inception_score

    def rejected(*args):
        rc = f(*args)
        msg = lib.dmvae_last_error()
        assert rc == -22 and b"inception_score" in msg, (rc, msg)
        return msg
    #   logits, dtype, n, classes, ld, order, splits, workspace, scores, stream
    for i in (0, 7, 8):                                                           # each pointer that must be there (order may be NULL)
        a = [p, 0, 100, 8, 8, None, 10, p, p]
        a[i] = None
        assert b"NULL" in rejected(*a, None)
    for dt in (-1, 3):
        assert b"dtype" in rejected(p, dt, 100, 8, 8, None, 10, p, p, None)
    for c in (1, 0, -4, 65537):
        assert b"classes" in rejected(p, 0, 100, c, 65537, None, 10, p, p, None)
    assert b"n must" in rejected(p, 0, 0, 8, 8, None, 1, p, p, None)
    assert b"n must" in rejected(p, 0, 1 << 31, 8, 8, None, 10, p, p, None)
    assert b"splits" in rejected(p, 0, 100, 8, 8, None, 0, p, p, None)
    assert b"splits" in rejected(p, 1, 100, 8, 8, p, 101, p, p, None)
    assert b"leading dimension" in rejected(p, 2, 100, 8, 7, None, 10, p, p, None)
    assert lib.dmvae_abi_version() == 9


def test_ops_refuse_cpu_tensors():
    import torch
    from dmvae_amd import _lib, ops
    with pytest.raises(_lib.DmvaeHipError):
        ops.resize_tf1_bilinear(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), 8)
    with pytest.raises(_lib.DmvaeHipError):
        ops.inception_score(torch.zeros(10, 8), splits=2)
