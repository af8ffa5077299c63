"""CPU: the decoder AttnBlock's streaming attention BACKWARD entry (csrc/attention_wide_bwd.hip, one head of 512 channels; reference: autograd of
models/flux_ae.py:37-49) is exported and bound, and validates its arguments before any HIP call -- errno-style code plus a message that carries the entry's name, no
GPU touched.  The entry is additive: the ABI version does not move."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

ENTRY = "dmvae_attention_wide_bwd_stream_bf16"


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_wide_bwd_entry_is_exported_and_bound(lib):
    from dmvae_amd import _lib, functional, ops
    assert ENTRY in _lib.SIGNATURES
    assert hasattr(lib, ENTRY)
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    assert restype is ctypes.c_int and len(argtypes) == 15       # q, k, v, o, dout, lse, dq, dk, dv, delta, batch, seq, channels, scale, stream
    assert argtypes[:10] == [ctypes.c_void_p] * 10 and argtypes[10:13] == [ctypes.c_int] * 3 and argtypes[13] is ctypes.c_float
    assert lib.dmvae_abi_version() == 9
    assert callable(ops.attention_wide_bwd_stream)
    assert functional.ATTN_WIDE_BWD_STREAM is None and functional.ATTN_WIDE_STREAM is None


def test_wide_bwd_route_rule_without_gpu(monkeypatch):
    """functional._attn_wide_bwd_stream: by default exactly behind a forward that streamed by its own default rule; a forced forward keeps the composed backward
    unless the backward switch says otherwise; a composed forward never has a streaming backward."""
    from dmvae_amd import functional as Fn
    assert Fn._attn_wide_bwd_stream(1156, 512, True) and not Fn._attn_wide_bwd_stream(1156, 512, False)
    assert not Fn._attn_wide_bwd_stream(1156, 256, True)
    monkeypatch.setattr(Fn, "ATTN_WIDE_STREAM", True)
    assert not Fn._attn_wide_bwd_stream(1156, 512, True)           # the pinned combination
    monkeypatch.setattr(Fn, "ATTN_WIDE_BWD_STREAM", True)
    assert Fn._attn_wide_bwd_stream(1156, 512, True) and Fn._attn_wide_bwd_stream(1024, 512, True)
    assert not Fn._attn_wide_bwd_stream(1156, 512, False)          # a composed forward saved P and has no lse
    monkeypatch.setattr(Fn, "ATTN_WIDE_STREAM", None)
    monkeypatch.setattr(Fn, "ATTN_WIDE_BWD_STREAM", False)
    assert not Fn._attn_wide_bwd_stream(1156, 512, True)


def test_wide_bwd_entry_rejects_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = getattr(lib, ENTRY)
    scale = 512 ** -0.5
    ptrs = [p] * 10

    def rejected(*args):
        rc = f(*args)
        msg = lib.dmvae_last_error()
        assert rc == -22 and b"attention_wide_bwd_stream_bf16" in msg, (rc, msg)
        return msg

    assert b"channels 512" in rejected(*ptrs, 1, 1156, 256, scale, None)       # another width
    assert b"channels 512" in rejected(*ptrs, 1, 1156, 520, scale, None)
    assert b"seq" in rejected(*ptrs, 1, 0, 512, scale, None)                   # seq 0
    rejected(*ptrs, 1, -5, 512, scale, None)
    for i in range(10):                                                        # each null operand: q, k, v, o, dout, lse, dq, dk, dv, delta
        assert b"null" in rejected(*[None if j == i else p for j in range(10)], 1, 1156, 512, scale, None), i
    rejected(*ptrs, 0, 1156, 512, scale, None)                                 # empty batch
    rejected(*ptrs, 1, 1156, 512, 0.0, None)                                   # the forward takes its row maximum on the raw scores: scale > 0
    rejected(*ptrs, 1, 1156, 512, float("nan"), None)
    assert b"grid" in rejected(*ptrs, 1 << 20, 1 << 20, 512, scale, None)      # more workgroups than a grid dimension holds
    assert lib.dmvae_abi_version() == 9
