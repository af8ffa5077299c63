"""CPU: the six entry points of csrc/manifold.hip are exported and bound, the three workspace sizes are their closed forms, and every entry validates its
arguments before any HIP call -- -22 plus a message that carries the entry's name, no GPU touched.  The entries are additive: the ABI version does not move."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

ENTRIES = {"dmvae_knn_radius_workspace": 1, "dmvae_knn_radius": 9, "dmvae_manifold_member_workspace": 2, "dmvae_manifold_member": 12,
           "dmvae_kid_mmd2_workspace": 2, "dmvae_kid_mmd2": 18}


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def _splits(rows, cols):
    rb, ct = -(-rows // 64), -(-cols // 64)
    return max(1, min(ct, -(-512 // rb)))


def test_manifold_entries_are_exported_and_bound(lib):
    from dmvae_amd import _lib
    for name, nargs in ENTRIES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert _lib.SIGNATURES[name][0] is (ctypes.c_size_t if name.endswith("_workspace") else ctypes.c_int), name
    assert lib.dmvae_abi_version() == 9 and _lib.ABI_VERSION == 9
    with open(os.path.join(ROOT, "include", "dmvae_hip.h")) as fh:
        header = fh.read()
    assert "size_t dmvae_knn_radius_workspace(size_t n);" in header
    assert "int dmvae_knn_radius(const void* x, int dtype, size_t n, int f, size_t ld, int k, void* workspace, double* radius2, dmvae_stream_t stream);" in header
    assert "size_t dmvae_manifold_member_workspace(size_t nq, size_t nr);" in header
    assert "int dmvae_manifold_member(const void* q, size_t nq, size_t ldq, const void* r, size_t nr, size_t ldr, int dtype, int f, const double* radius2," in header
    assert "size_t dmvae_kid_mmd2_workspace(size_t subsets, size_t m);" in header
    assert "int dmvae_kid_mmd2(const void* x, size_t n1, size_t ldx, const void* y, size_t n2, size_t ldy, int dtype, int f, const int64_t* idx1," in header
    for ref in ("sample_50k.py:185-199", "evaluation/fid.py:15-45"):
        assert header.count(ref) >= 6, ref


def test_workspaces_are_their_closed_forms(lib):
    knn, mem, kid = lib.dmvae_knn_radius_workspace, lib.dmvae_manifold_member_workspace, lib.dmvae_kid_mmd2_workspace
    for n in (2, 9, 64, 65, 130, 2049, 10000, 32768, 32769, 50000, (1 << 30) - 64):
        assert knn(n) == (n + _splits(n, n) * n * 9) * 8, n
    assert knn(50000) == (50000 + 50000 * 9) * 8 and knn(2049) == (2049 + 16 * 2049 * 9) * 8 and knn(64) == (64 + 64 * 9) * 8
    assert knn(0) == 0 and knn(1) == 0 and knn(1 << 31) == 0 and knn((1 << 30) - 63) == 0      # beyond 2^24 - 1 row blocks no launch could take them
    for nq, nr in ((1, 1), (9, 130), (130, 9), (2049, 2049), (10000, 50000), (50000, 10000), (50000, 50000)):
        assert mem(nq, nr) == (nq + nr) * 8 + -(-(_splits(nq, nr) * nq) // 8) * 8, (nq, nr)
    assert mem(9, 130) == 139 * 8 + 32 and mem(50000, 50000) == 800000 + 50000
    assert mem(0, 5) == 0 and mem(5, 0) == 0 and mem(1 << 31, 5) == 0 and mem(5, 1 << 31) == 0 and mem((1 << 30) - 63, 5) == 0 and mem(5, (1 << 30) - 63) == 0
    assert mem((1 << 30) - 64, 5) == ((1 << 30) - 59) * 8 + (1 << 30) - 64
    for s, m in ((1, 2), (4, 16), (3, 65), (100, 1000), (7, 1 << 15)):
        assert kid(s, m) == s * 3 * (-(-m // 64)) ** 2 * 8, (s, m)
    assert kid(100, 1000) == 100 * 3 * 256 * 8
    assert kid(0, 16) == 0 and kid(4, 1) == 0 and kid(4, 0) == 0 and kid(4, (1 << 20) + 1) == 0 and kid(1 << 20, 1 << 20) == 0
    # one launch takes 2^24 - 1 workgroups: 21845 x 3 x 16^2 = 2^24 - 256 tiles fit, 21846 subsets do not
    assert kid(21845, 1000) == 21845 * 3 * 256 * 8 and kid(21846, 1000) == 0 and kid(1 << 24, 2) == 0


def _rejecter(lib, f, name):
    def rejected(*args):
        rc = f(*args)
        msg = lib.dmvae_last_error()
        assert rc == -22 and name in msg, (rc, msg)
        return msg
    return rejected


def test_knn_radius_rejects_bad_arguments_without_gpu(lib):
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    rejected = _rejecter(lib, lib.dmvae_knn_radius, b"knn_radius")
    #   x, dtype, n, f, ld, k, workspace, radius2, stream
    for i in (0, 6, 7):
        a = [p, 0, 100, 16, 16, 3, p, p]
        a[i] = None
        assert b"NULL" in rejected(*a, None)
    for dt in (-1, 1, 3):                                                         # bf16 (1) is not a feature dtype here
        assert b"dtype" in rejected(p, dt, 100, 16, 16, 3, p, p, None)
    for f in (0, 8, 24, 4112, -16):
        assert b"f must" in rejected(p, 0, 100, f, 8192, 3, p, p, None)
    for k in (0, 9, -1):
        assert b"k must" in rejected(p, 0, 100, 16, 16, k, p, p, None)
    for n, k in ((0, 1), (1, 1), (3, 3), (8, 8), (1 << 31, 3), ((1 << 30) - 63, 3)):                  # N <= k has no k-th neighbour
        assert b"n must" in rejected(p, 2, n, 16, 16, k, p, p, None)
    assert b"leading dimension" in rejected(p, 0, 100, 48, 47, 3, p, p, None)
    assert lib.dmvae_abi_version() == 9


def test_manifold_member_rejects_bad_arguments_without_gpu(lib):
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    rejected = _rejecter(lib, lib.dmvae_manifold_member, b"manifold_member")
    #   q, nq, ldq, r, nr, ldr, dtype, f, radius2, workspace, member, stream
    for i in (0, 3, 8, 9, 10):
        a = [p, 10, 16, p, 20, 16, 0, 16, p, p, p]
        a[i] = None
        assert b"NULL" in rejected(*a, None)
    for dt in (-1, 1, 3):
        assert b"dtype" in rejected(p, 10, 16, p, 20, 16, dt, 16, p, p, p, None)
    for f in (0, 8, 40, 4112):
        assert b"f must" in rejected(p, 10, 8192, p, 20, 8192, 0, f, p, p, p, None)
    assert b"nq and nr" in rejected(p, 0, 16, p, 20, 16, 0, 16, p, p, p, None)
    assert b"nq and nr" in rejected(p, 10, 16, p, 0, 16, 2, 16, p, p, p, None)
    assert b"nq and nr" in rejected(p, 1 << 31, 16, p, 20, 16, 2, 16, p, p, p, None)
    assert b"nq and nr" in rejected(p, (1 << 30) - 63, 16, p, 20, 16, 2, 16, p, p, p, None)
    assert b"nq and nr" in rejected(p, 10, 16, p, (1 << 30) - 63, 16, 2, 16, p, p, p, None)
    assert b"leading dimension" in rejected(p, 10, 15, p, 20, 16, 0, 16, p, p, p, None)
    assert b"leading dimension" in rejected(p, 10, 16, p, 20, 15, 0, 16, p, p, p, None)
    assert lib.dmvae_abi_version() == 9


def test_kid_mmd2_rejects_bad_arguments_without_gpu(lib):
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    rejected = _rejecter(lib, lib.dmvae_kid_mmd2, b"kid_mmd2")
    #   x, n1, ldx, y, n2, ldy, dtype, f, idx1, idx2, subsets, m, degree, gamma, coef0, workspace, mmd2, stream
    good = [p, 100, 16, p, 90, 16, 0, 16, p, p, 4, 16, 3, 1 / 16, 1.0, p, p]
    for i in (0, 3, 8, 9, 15, 16):
        a = list(good)
        a[i] = None
        assert b"NULL" in rejected(*a, None)

    def with_(**kw):
        names = ["x", "n1", "ldx", "y", "n2", "ldy", "dtype", "f", "idx1", "idx2", "subsets", "m", "degree", "gamma", "coef0", "ws", "out"]
        a = list(good)
        for key, v in kw.items():
            a[names.index(key)] = v
        return rejected(*a, None)
    for dt in (-1, 1, 3):
        assert b"dtype" in with_(dtype=dt)
    for f in (0, 8, 24, 4112):
        assert b"f must" in with_(f=f, ldx=8192, ldy=8192)
    for m in (0, 1, (1 << 20) + 1):
        assert b"m must" in with_(m=m)
    assert b"n1 and n2" in with_(n1=15) and b"n1 and n2" in with_(n2=15) and b"n1 and n2" in with_(n1=1 << 31) and b"n1 and n2" in with_(n2=(1 << 30) - 63)
    assert b"subsets" in with_(subsets=0) and b"subsets" in with_(subsets=5592406)                  # 5592406 x 3 tiles of one block: 2^24 + 2
    for d in (0, 9, -3):
        assert b"degree" in with_(degree=d)
    assert b"leading dimension" in with_(ldx=15) and b"leading dimension" in with_(ldy=15)
    assert lib.dmvae_abi_version() == 9


def test_ops_refuse_cpu_tensors():
    import torch
    from dmvae_amd import _lib, ops
    x, r2 = torch.zeros(10, 16), torch.zeros(10, dtype=torch.float64)
    idx = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(_lib.DmvaeHipError):
        ops.knn_radius(x, 3)
    with pytest.raises(_lib.DmvaeHipError):
        ops.manifold_member(x, x, r2)
    with pytest.raises(_lib.DmvaeHipError):
        ops.kid_mmd2(x, x, idx, idx)
