#!/usr/bin/env python
"""Every call the nine attention entries reject on the host, with its return code and dmvae_last_error() text, one line each -- to diff two builds of the
library (DMVAE_LIB=/path/to/other/libdmvae_hip.so python tools/attention_rejections.py > other.txt).  No GPU: validation returns before any HIP call.
The streaming entries get the rejecting calls of tests/test_attention_{stream,bwd_stream,heads_stream}_abi.py, the resident ones a null operand, seq 0, seq 289,
head dim 60 and a bad padded width."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dmvae_amd import _lib

lib = _lib.lib()
buf = ctypes.create_string_buffer(64)
p = ctypes.cast(buf, ctypes.c_void_p)
inf, nan = float("inf"), float("nan")


def show(a):
    return "p" if a is p else repr(a)


def each(name, nptr, tails):
    """`name` with nptr non-null pointers followed by each of `tails` (and a null stream)"""
    f = getattr(lib, "dmvae_" + name)
    for t in tails:
        args = [p] * nptr + list(t)
        rc = f(*args, None)
        print(f"{name}({', '.join(show(a) for a in args)}) -> {rc} {lib.dmvae_last_error().decode()!r}")
        assert rc != 0, "accepted: the call would have reached the GPU"


def call(name, nptr, *tail):
    """`name` with each of its nptr leading pointers null in turn"""
    each(name, 0, [tuple(None if j == i else p for j in range(nptr)) + tail for i in range(nptr)])


s64, s72 = 64 ** -0.5, 72 ** -0.5
# ---- streaming, packed qkv: (batch, seq, heads, head_dim, scale)
bad_qkv = [(1, 300, 2, 72, s64), (1, 0, 2, 64, s64), (1, -5, 2, 64, s64), (0, 300, 2, 64, s64), (1, 300, 0, 64, s64), (1, 300, 2, 64, 0.0), (1, 300, 2, 64, -0.125),
           (1, 300, 2, 64, nan), (1, 300, 2, 64, inf), (1 << 20, 1 << 20, 1 << 10, 64, s64), (1, 300, 1 << 24, 64, s64)]
for i in range(2):      # qkv, out (lse is optional)
    each("attention_qkv_stream_bf16", 0, [tuple(None if j == i else p for j in range(2)) + (None, 1, 300, 2, 64, s64)])
each("attention_qkv_stream_bf16", 0, [(p, p, None) + t for t in bad_qkv])
call("attention_bwd_qkv_stream_bf16", 6, 1, 300, 2, 64, s64)
each("attention_bwd_qkv_stream_bf16", 6, bad_qkv)
# ---- streaming, head-major: (batch, seq, heads, head_dim, head_dim_padded, scale)
bad_heads = [(0, 300, 2, 72, 72, s72), (1, 300, 0, 72, 72, s72), (1, 0, 2, 72, 72, s72), (1, -5, 2, 72, 72, s72)]
bad_heads += [(1, 300, 2, d, (d + 31) // 32 * 32, s72) for d in (32, 40, 80, 96, 128)]
bad_heads += [(1, 300, 2, d, dp, s72) for d, dp in ((72, 64), (72, 80), (72, 128), (64, 96), (64, 72), (64, 0))]
bad_heads += [(1, 300, 2, d, dp, s) for d, dp in ((72, 96), (64, 64)) for s in (0.0, -s72, nan, inf)]
bad_heads += [(1 << 20, 1 << 20, 1 << 10, 72, 96, s72), (1 << 20, 1 << 20, 1 << 10, 64, 64, s72)]
for i in range(4):      # q, k, v, out (lse is optional)
    each("attention_heads_stream_bf16", 0, [tuple(None if j == i else p for j in range(4)) + (None, 1, 300, 2, 72, 72, s72)])
each("attention_heads_stream_bf16", 0, [(p, p, p, p, None) + t for t in bad_heads])
call("attention_bwd_heads_stream_bf16", 10, 1, 300, 2, 72, 72, s72)
each("attention_bwd_heads_stream_bf16", 10, bad_heads)
# ---- resident: a null operand, seq 0, seq 289, head dim 60, a bad padded width
res_qkv = [(1, 0, 2, 64, s64), (1, 289, 2, 64, s64), (1, 100, 2, 60, s64), (0, 100, 2, 64, s64), (1, 100, 0, 64, s64)]
res_heads = [(1, 0, 2, 72, 96, s72), (1, 289, 2, 72, 96, s72), (1, 100, 2, 60, 64, s72), (1, 100, 2, 72, 80, s72), (1, 100, 2, 72, 64, s72), (1, 100, 2, 104, 104, s72),
             (1, 100, 2, 64, 0, s72)]
call("attention_qkv_lse_bf16", 2, None, 1, 100, 2, 64, s64)
each("attention_qkv_lse_bf16", 0, [(p, p, None) + t for t in res_qkv])
call("attention_heads_lse_bf16", 4, None, 1, 100, 2, 72, 96, s72)
each("attention_heads_lse_bf16", 0, [(p, p, p, p, None) + t for t in res_heads])
call("attention_qknorm_rope_bf16", 6, 1, 100, 2, 72, 1e-6, s72)
each("attention_qknorm_rope_bf16", 6, [t[:4] + (1e-6, t[4]) for t in res_qkv[:2] + [(1, 100, 2, 60, s64), (1, 100, 2, 104, s64), (1, 100, 2, 0, s64)] + res_qkv[3:]])
for i in (0, 1, 2, 4):      # qkv, out, dout, dqkv (lse is optional)
    each("attention_bwd_qkv_lse_bf16", 0, [tuple(None if j == i else p for j in range(5)) + (1, 100, 2, 64, s64)])
each("attention_bwd_qkv_lse_bf16", 5, res_qkv)
for i in (0, 1, 2, 3, 4, 6, 7, 8):      # q, k, v, out, dout, dq, dk, dv (lse is optional)
    each("attention_bwd_heads_lse_bf16", 0, [tuple(None if j == i else p for j in range(9)) + (1, 100, 2, 72, 96, s72)])
each("attention_bwd_heads_lse_bf16", 9, res_heads)
