"""CPU: the entry points of csrc/dit_variants.hip (LayerNorm + modulate forward / backward, the head split of the block variants, tanh-GELU) are exported and
bound, and validate their arguments before any HIP call -- -22 plus a message that carries the entry's name, no GPU touched.  The entries are additive: the ABI
version does not move."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

ENTRIES = {"dmvae_layernorm_modulate_bf16": 11, "dmvae_gated_residual_layernorm_modulate": 16, "dmvae_layernorm_modulate_bwd_workspace": 3,
           "dmvae_layernorm_modulate_bwd": 15, "dmvae_head_split_bf16": 17, "dmvae_head_split_bwd_nblk": 3, "dmvae_head_split_bwd": 23,
           "dmvae_gelu_tanh_fwd": 4, "dmvae_gelu_tanh_bwd": 5}


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "dmvae_amd", "csrc"), "-j8"], check=True)
    return _lib.lib()


def test_variant_entries_are_exported_and_bound(lib):
    from dmvae_amd import _lib
    for name, nargs in ENTRIES.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.dmvae_abi_version() == 9 and _lib.ABI_VERSION == 9
    # the workspace queries: the partial sums [B][32][2][C] f32 and two float4 per row; one [2][D] f32 row per first-stage block
    assert lib.dmvae_layernorm_modulate_bwd_workspace(3, 64, 1152) == 3 * 32 * 2 * 1152 * 4 + 3 * 64 * 32
    assert lib.dmvae_layernorm_modulate_bwd_workspace(0, 64, 1152) == 0
    assert lib.dmvae_head_split_bwd_nblk(3, 64, 3) == 144 and lib.dmvae_head_split_bwd_nblk(16, 256, 16) == 2048 and lib.dmvae_head_split_bwd_nblk(1, 1, 1) == 1


def _rejecter(lib, name):
    f = getattr(lib, name)

    def rejected(*args):
        rc = f(*args)
        msg = lib.dmvae_last_error()
        assert rc == -22 and name[len("dmvae_"):].encode() in msg, (rc, msg)
        return msg
    return rejected


def test_layernorm_entries_reject_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    c = 1152
    fwd = _rejecter(lib, "dmvae_layernorm_modulate_bf16")
    #   x, mod, y, rows, rows_per_sample, c, mod_stride, shift_off, scale_off, eps, stream
    assert b"2048" in fwd(p, p, p, 8, 4, 2052, 6 * 2052, 0, 2052, 1e-6, None)                 # width > 2048
    assert b"multiple of 4" in fwd(p, p, p, 8, 4, 1150, 6 * 1150, 0, 1150, 1e-6, None)        # width % 4
    assert b"offsets" in fwd(p, p, p, 8, 4, c, 6 * c, 0, 5 * c + 4, 1e-6, None)               # the scale chunk runs past the stride
    assert b"offsets" in fwd(p, p, p, 8, 4, c, 6 * c, 5 * c + 4, c, 1e-6, None)               # the shift chunk does
    assert b"offsets" in fwd(p, p, p, 8, 4, c, 6 * c, 2, c, 1e-6, None)                       # offsets % 4
    assert b"offsets" in fwd(p, p, p, 8, 4, c, 4 * c, -1, -4, 1e-6, None)                     # only the shift may be absent
    for i in range(3):                                                                        # each null pointer
        a = [None if j == i else p for j in range(3)]
        fwd(*a, 8, 4, c, 6 * c, 0, c, 1e-6, None)
    fwd(p, p, p, 0, 4, c, 6 * c, 0, c, 1e-6, None)
    fwd(p, p, p, 8, 0, c, 6 * c, 0, c, 1e-6, None)
    res = _rejecter(lib, "dmvae_gated_residual_layernorm_modulate")
    #   x_in, x_out, r, gate_mod, gate_stride, gate_off, mod, y, rows, rows_per_sample, c, mod_stride, shift_off, scale_off, eps, stream
    assert b"2048" in res(p, p, p, p, 6 * 2052, 0, p, p, 8, 4, 2052, 6 * 2052, 0, 2052, 1e-6, None)
    assert b"multiple of 4" in res(p, p, p, p, 6 * c, 0, p, p, 8, 4, 1150, 6 * c, 0, c, 1e-6, None)
    assert b"offsets" in res(p, p, p, p, 4 * c, 3 * c + 4, p, p, 8, 4, c, 4 * c, -1, 2 * c, 1e-6, None)      # the gate chunk runs past its stride
    assert b"offsets" in res(p, p, p, p, 4 * c, 3 * c, p, p, 8, 4, c, 4 * c, -1, 3 * c + 4, 1e-6, None)
    for i in (0, 1, 2, 3, 6, 7):
        a = [p, p, p, p, 6 * c, 2 * c, p, p]
        a[i] = None
        res(*a, 8, 4, c, 6 * c, 3 * c, 4 * c, 1e-6, None)
    bwd = _rejecter(lib, "dmvae_layernorm_modulate_bwd")
    #   da, x, mod, dx_io, dmod, workspace, workspace_bytes, batch, seq, c, mod_stride, shift_off, scale_off, eps, stream
    need = lib.dmvae_layernorm_modulate_bwd_workspace(3, 64, c)
    assert b"workspace too small" in bwd(p, p, p, p, p, p, need - 1, 3, 64, c, 6 * c, 0, c, 1e-6, None)
    assert b"2048" in bwd(p, p, p, p, p, p, 1 << 30, 3, 64, 2052, 6 * 2052, 0, 2052, 1e-6, None)
    assert b"multiple of 4" in bwd(p, p, p, p, p, p, 1 << 30, 3, 64, 1150, 6 * c, 0, c, 1e-6, None)
    assert b"offsets" in bwd(p, p, p, p, p, p, need, 3, 64, c, 4 * c, -1, 3 * c + 4, 1e-6, None)
    for i in range(6):
        a = [None if j == i else p for j in range(6)]
        bwd(*a, need, 3, 64, c, 6 * c, 0, c, 1e-6, None)
    bwd(p, p, p, p, p, p, need, 0, 64, c, 6 * c, 0, c, 1e-6, None)
    assert lib.dmvae_abi_version() == 9


def test_head_split_and_gelu_entries_reject_bad_arguments_without_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = _rejecter(lib, "dmvae_head_split_bf16")
    #   qkv, q_weight, k_weight, cos, sin, q_out, k_out, v_out, batch, seq, heads, head_dim, head_dim_padded, norm_kind, rope, eps, stream
    assert b"head dim" in fwd(p, None, None, None, None, p, p, p, 2, 64, 3, 63, 64, 0, 0, 1e-6, None)          # odd head dim
    assert b"head dim" in fwd(p, None, None, None, None, p, p, p, 2, 64, 3, 64, 160, 0, 0, 1e-6, None)         # padded head dim > 128
    assert b"head dim" in fwd(p, None, None, None, None, p, p, p, 2, 64, 3, 72, 64, 0, 0, 1e-6, None)          # padded < head dim
    assert b"norm kind" in fwd(p, p, p, p, p, p, p, p, 2, 64, 3, 64, 64, 2, 1, 1e-6, None)                     # 2 would be the LayerNorm kind: not built
    assert b"null" in fwd(p, None, p, None, None, p, p, p, 2, 64, 3, 64, 64, 1, 0, 1e-6, None)                 # rms without its weight
    assert b"null" in fwd(p, None, None, p, None, p, p, p, 2, 64, 3, 64, 64, 0, 1, 1e-6, None)                 # rope without its table
    for i in (0, 5, 6, 7):
        a = [p, None, None, None, None, p, p, p]
        a[i] = None
        fwd(*a, 2, 64, 3, 64, 64, 0, 0, 1e-6, None)
    fwd(p, None, None, None, None, p, p, p, 0, 64, 3, 64, 64, 0, 0, 1e-6, None)
    assert b"rows" in fwd(p, None, None, None, None, p, p, p, 1 << 15, 1 << 15, 16, 64, 64, 0, 0, 1e-6, None)  # more rows than the grid's index holds
    bwd = _rejecter(lib, "dmvae_head_split_bwd")
    #   dq, dk, dv, qkv, q_weight, k_weight, cos, sin, dqkv, dq_weight, dk_weight, workspace, workspace_bytes, batch, seq, heads, d, dp, norm_kind, rope, eps, acc, stream
    need = lib.dmvae_head_split_bwd_nblk(2, 64, 3) * 2 * 64 * 4
    assert b"workspace too small" in bwd(p, p, p, p, p, p, None, None, p, p, p, p, need - 1, 2, 64, 3, 64, 64, 1, 0, 1e-6, 0, None)
    assert b"workspace too small" in bwd(p, p, p, p, p, p, None, None, p, p, p, None, need, 2, 64, 3, 64, 64, 1, 0, 1e-6, 0, None)
    assert b"together" in bwd(p, p, p, p, p, p, None, None, p, p, None, p, need, 2, 64, 3, 64, 64, 1, 0, 1e-6, 0, None)       # one weight gradient without the other
    assert b"together" in bwd(p, p, p, p, None, None, None, None, p, p, p, p, need, 2, 64, 3, 64, 64, 0, 0, 1e-6, 0, None)    # weight gradients without a norm
    assert b"head dim" in bwd(p, p, p, p, None, None, None, None, p, None, None, None, 0, 2, 64, 3, 63, 64, 0, 0, 1e-6, 0, None)
    assert b"null" in bwd(p, p, p, None, p, p, None, None, p, None, None, None, 0, 2, 64, 3, 64, 64, 1, 0, 1e-6, 0, None)     # rms needs the forward's qkv
    for i in (0, 1, 2, 8):
        a = [p, p, p, p, None, None, None, None, p]
        a[i] = None
        bwd(*a, None, None, None, 0, 2, 64, 3, 64, 64, 0, 0, 1e-6, 0, None)
    for name, n_ptr in (("dmvae_gelu_tanh_fwd", 2), ("dmvae_gelu_tanh_bwd", 3)):
        rej = _rejecter(lib, name)
        for i in range(n_ptr):
            assert b"null" in rej(*[None if j == i else p for j in range(n_ptr)], 8, None)
    assert lib.dmvae_gelu_tanh_fwd(p, p, 0, None) == 0 and lib.dmvae_gelu_tanh_bwd(p, p, p, 0, None) == 0      # nothing to do: no launch
    assert lib.dmvae_abi_version() == 9
