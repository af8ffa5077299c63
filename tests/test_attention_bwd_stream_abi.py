"""CPU: the streaming attention backward entry (csrc/attention_bwd_stream.hip) is exported and bound, and validates its arguments before any HIP call --
errno-style code plus a message, no GPU touched.  The entry is additive: the ABI version does not move."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_stream_backward_entry_is_exported_and_bound(lib):
    from dmvae_amd import _lib
    c_void_p = ctypes.c_void_p
    assert "dmvae_attention_bwd_qkv_stream_bf16" in _lib.SIGNATURES
    assert hasattr(lib, "dmvae_attention_bwd_qkv_stream_bf16")
    res, args = _lib.SIGNATURES["dmvae_attention_bwd_qkv_stream_bf16"]
    res0, args0 = _lib.SIGNATURES["dmvae_attention_bwd_qkv_lse_bf16"]
    assert res == res0 and args == args0[:5] + [c_void_p] + args0[5:]      # the resident entry's operands plus the delta scratch behind dqkv
    assert lib.dmvae_abi_version() == 9


def test_stream_backward_entry_rejects_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.dmvae_attention_bwd_qkv_stream_bf16
    scale = 64 ** -0.5

    def rejected(*args):
        rc = f(*args)
        msg = lib.dmvae_last_error()
        assert rc != 0 and b"attention_bwd_qkv_stream_bf16" in msg, (rc, msg)
        return msg

    for i in range(6):                                                                      # qkv, out, dout, lse, dqkv, delta: none may be null
        ptrs = [p] * 6
        ptrs[i] = None
        assert b"null" in rejected(*ptrs, 1, 300, 2, 64, scale, None), i
    assert b"lse" in rejected(p, p, p, None, p, p, 1, 300, 2, 64, scale, None)              # the row statistics are required
    assert b"head_dim 64" in rejected(p, p, p, p, p, p, 1, 300, 2, 72, scale, None)         # head_dim 72
    assert b"seq" in rejected(p, p, p, p, p, p, 1, 0, 2, 64, scale, None)                   # seq 0
    rejected(p, p, p, p, p, p, 1, -5, 2, 64, scale, None)
    rejected(p, p, p, p, p, p, 0, 300, 2, 64, scale, None)                                  # empty batch
    rejected(p, p, p, p, p, p, 1, 300, 0, 64, scale, None)                                  # no heads
    rejected(p, p, p, p, p, p, 1, 300, 2, 64, 0.0, None)                                    # scale > 0
    rejected(p, p, p, p, p, p, 1, 300, 2, 64, -0.125, None)
    rejected(p, p, p, p, p, p, 1, 300, 2, 64, float("nan"), None)
    rejected(p, p, p, p, p, p, 1, 300, 2, 64, float("inf"), None)
    rejected(p, p, p, p, p, p, 1 << 20, 1 << 20, 1 << 10, 64, scale, None)                  # more workgroups than a grid dimension holds
    rejected(p, p, p, p, p, p, 1, 300, 1 << 24, 64, scale, None)                            # a token row stride past int
    assert lib.dmvae_abi_version() == 9
