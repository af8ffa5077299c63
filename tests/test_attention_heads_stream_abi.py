"""CPU: the head-major streaming attention entries (csrc/attention_stream.hip, csrc/attention_bwd_stream.hip: LightningDiT's attention beyond 288 tokens) are
exported and bound, and validate their arguments before any HIP call -- errno-style code plus a message that names the entry, no GPU touched.  The entries are
additive: the ABI version does not move."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

FWD, BWD = "dmvae_attention_heads_stream_bf16", "dmvae_attention_bwd_heads_stream_bf16"


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_heads_stream_entries_are_exported_and_bound(lib):
    from dmvae_amd import _lib
    for name in (FWD, BWD):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES[FWD] == _lib.SIGNATURES["dmvae_attention_heads_lse_bf16"]            # same operands as the resident entry
    res, args = _lib.SIGNATURES["dmvae_attention_bwd_heads_lse_bf16"]
    assert _lib.SIGNATURES[BWD] == (res, args[:9] + [ctypes.c_void_p] + args[9:])               # the resident entry plus `delta`
    assert lib.dmvae_abi_version() == 9


def _rejecting(lib, f, name):
    def rejected(*args):
        rc = f(*args)
        msg = lib.dmvae_last_error()
        assert rc != 0 and name in msg, (rc, msg)
        return msg
    return rejected


def test_heads_stream_forward_rejects_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rejected = _rejecting(lib, getattr(lib, FWD), b"attention_heads_stream_bf16")
    scale = 72 ** -0.5
    for i in range(4):                                                               # null q, k, v, out (lse is optional)
        ptrs = [p] * 4
        ptrs[i] = None
        assert b"null" in rejected(*ptrs, None, 1, 300, 2, 72, 72, scale, None)
    rejected(p, p, p, p, None, 0, 300, 2, 72, 72, scale, None)                       # empty batch
    rejected(p, p, p, p, None, 1, 300, 0, 72, 72, scale, None)                       # no heads
    assert b"seq" in rejected(p, p, p, p, None, 1, 0, 2, 72, 72, scale, None)        # seq 0
    rejected(p, p, p, p, None, 1, -5, 2, 72, 72, scale, None)
    for d in (32, 40, 80, 96, 128):                                                  # head dims other than 64 and 72
        assert b"head_dim 64 or 72" in rejected(p, p, p, p, None, 1, 300, 2, d, (d + 31) // 32 * 32, scale, None)
    for d, dp in ((72, 64), (72, 80), (72, 128), (64, 96), (64, 72), (64, 0)):       # q / k rows that are neither head_dim nor its round-up to 32
        assert b"rounded up to 32" in rejected(p, p, p, p, None, 1, 300, 2, d, dp, scale, None)
    rejected(p, p, p, p, None, 1, 300, 2, 72, 96, 0.0, None)                         # the row maximum is taken on the raw scores: scale > 0
    rejected(p, p, p, p, None, 1, 300, 2, 72, 96, -scale, None)
    rejected(p, p, p, p, None, 1, 300, 2, 72, 96, float("nan"), None)
    rejected(p, p, p, p, None, 1, 300, 2, 72, 96, float("inf"), None)
    assert b"grid" in rejected(p, p, p, p, None, 1 << 20, 1 << 20, 1 << 10, 72, 96, scale, None)      # more workgroups than a grid dimension holds
    assert lib.dmvae_abi_version() == 9


def test_heads_stream_backward_rejects_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    rejected = _rejecting(lib, getattr(lib, BWD), b"attention_bwd_heads_stream_bf16")
    scale = 72 ** -0.5
    for i in range(10):                                                              # q, k, v, out, dout, lse, dq, dk, dv, delta: every one is required
        ptrs = [p] * 10
        ptrs[i] = None
        msg = rejected(*ptrs, 1, 300, 2, 72, 72, scale, None)
        assert b"null" in msg and (i != 5 or b"lse" in msg) and (i != 9 or b"delta" in msg), msg
    ok = [p] * 10
    rejected(*ok, 0, 300, 2, 72, 72, scale, None)
    rejected(*ok, 1, 300, 0, 72, 72, scale, None)
    assert b"seq" in rejected(*ok, 1, 0, 2, 72, 72, scale, None)
    rejected(*ok, 1, -5, 2, 72, 72, scale, None)
    for d in (32, 40, 80, 96, 128):
        assert b"head_dim 64 or 72" in rejected(*ok, 1, 300, 2, d, (d + 31) // 32 * 32, scale, None)
    for d, dp in ((72, 64), (72, 80), (72, 128), (64, 96), (64, 72), (64, 0)):
        assert b"rounded up to 32" in rejected(*ok, 1, 300, 2, d, dp, scale, None)
    rejected(*ok, 1, 300, 2, 64, 64, 0.0, None)
    rejected(*ok, 1, 300, 2, 64, 64, -scale, None)
    rejected(*ok, 1, 300, 2, 64, 64, float("nan"), None)
    rejected(*ok, 1, 300, 2, 64, 64, float("inf"), None)
    assert b"grid" in rejected(*ok, 1 << 20, 1 << 20, 1 << 10, 72, 96, scale, None)
    assert lib.dmvae_abi_version() == 9
