"""CPU: the decoder AttnBlock's streaming attention entry (csrc/attention_wide.hip, one head of 512 channels; reference models/flux_ae.py:37-49) is exported and
bound, and validates its arguments before any HIP call -- errno-style code plus a message that carries the entry's name, no GPU touched.  The entry is additive: the
ABI version does not move.  And the decoder's token input: any square grid, anything else a ValueError ahead of every kernel."""
import ctypes
import os
import subprocess

import pytest
import torch

from conftest import ROOT

ENTRY = "dmvae_attention_wide_stream_bf16"


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_wide_entry_is_exported_and_bound(lib):
    from dmvae_amd import _lib, ops
    assert ENTRY in _lib.SIGNATURES
    assert hasattr(lib, ENTRY)
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    assert restype is ctypes.c_int and len(argtypes) == 10       # q, k, v, out, lse, batch, seq, channels, scale, stream
    assert lib.dmvae_abi_version() == 9
    assert ops.ATTNBLOCK_COMPOSED_MAX == 1024
    assert ops.attention_wide_supported(1, 512) and ops.attention_wide_supported(4096, 512)
    assert not ops.attention_wide_supported(4096, 256) and not ops.attention_wide_supported(0, 512)


def test_wide_entry_rejects_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = getattr(lib, ENTRY)
    scale = 512 ** -0.5

    def rejected(*args):
        rc = f(*args)
        msg = lib.dmvae_last_error()
        assert rc == -22 and b"attention_wide_stream_bf16" in msg, (rc, msg)
        return msg

    assert b"channels 512" in rejected(p, p, p, p, None, 1, 1156, 256, scale, None)       # another width
    assert b"channels 512" in rejected(p, p, p, p, None, 1, 1156, 520, scale, None)
    assert b"seq" in rejected(p, p, p, p, None, 1, 0, 512, scale, None)                   # seq 0
    rejected(p, p, p, p, None, 1, -5, 512, scale, None)
    for i in range(4):                                                                    # each null operand
        ops4 = [None if j == i else p for j in range(4)]
        assert b"null" in rejected(*ops4, None, 1, 1156, 512, scale, None)
    rejected(p, p, p, p, None, 0, 1156, 512, scale, None)                                 # empty batch
    rejected(p, p, p, p, None, 1, 1156, 512, 0.0, None)                                   # the row maximum is taken on the raw scores: scale > 0
    rejected(p, p, p, p, None, 1, 1156, 512, float("nan"), None)
    assert b"grid" in rejected(p, p, p, p, None, 1 << 20, 1 << 20, 512, scale, None)      # more workgroups than a grid dimension holds
    assert lib.dmvae_abi_version() == 9


def test_decoder_rejects_a_token_count_that_is_no_square_before_any_kernel():
    from dmvae_amd.models.flux_ae import Decoder
    dec = Decoder(ch=32, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, in_channels=3, resolution=32, z_channels=32)
    with pytest.raises(ValueError, match="square"):
        dec(torch.zeros(1, 300, 32))         # CPU tokens: a kernel call would raise DmvaeHipError instead
