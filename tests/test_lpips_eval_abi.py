"""CPU: the evaluation LPIPS' entry points (csrc/lpips_eval.hip) and the (11, 11) form of dmvae_conv2d_f32_fwd are declared, exported and bound, and refuse
everything outside their contract with -22 and a message before any launch (no GPU is touched: every call below returns from argument validation); the
workspace size is the closed form of include/dmvae_hip.h."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

ENTRY_POINTS = ("dmvae_lpips_input", "dmvae_lpips_head")


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(64)
    return ctypes.cast(buf, ctypes.c_void_p)


def test_entry_points_are_declared_exported_and_bound(lib):
    from dmvae_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} is not declared in include/dmvae_hip.h"
    assert re.search(r"\bsize_t dmvae_lpips_head_workspace\s*\(", hdr)
    for name in ENTRY_POINTS + ("dmvae_lpips_head_workspace",):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.dmvae_abi_version() == 9 and _lib.ABI_VERSION == 9                     # additions only
    assert callable(ops.lpips_input) and callable(ops.lpips_head)
    full = open(os.path.join(ROOT, "include", "dmvae_hip.h")).read()
    assert full.count("Reference: evaluation/metrics.py:26-29") >= 3


def conv11(lib, p, *, cin=3, cout=64, h=63, w=63, stride=4, ph=2, pw=2, kh=11, kw=11):
    return lib.dmvae_conv2d_f32_fwd(p, p, None, p, p, 1, h, w, cin, cout, kh, kw, stride, ph, pw, 1, 0, cout, None)


@pytest.mark.parametrize("kw_,needle", [
    (dict(stride=1), b"(11, 11)"),
    (dict(stride=2), b"(11, 11)"),
    (dict(ph=0, pw=0), b"(11, 11)"),
    (dict(ph=5, pw=5), b"(11, 11)"),
    (dict(cin=16), b"cin 3 only"),
    (dict(cin=64), b"cin 3 only"),
    (dict(cin=20), b"cin"),
    (dict(kh=11, kw=1), b"(11, 1)"),
    (dict(kh=1, kw=11), b"(1, 11)"),
    (dict(cout=24), b"cout must be a multiple of 16"),
    (dict(h=6, w=63), b"smaller than"),
])
def test_the_11x11_form_is_cin3_stride4_pad2_only(lib, p, kw_, needle):
    assert conv11(lib, p, **kw_) == -22
    assert needle in lib.dmvae_last_error(), lib.dmvae_last_error()


def test_input_refusals(lib, p):
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.dmvae_lpips_input(args[0], args[1], 0, args[2], 1, 8, 8, None) == -22 and b"NULL" in lib.dmvae_last_error()
    for b, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, 40000, 8)):
        assert lib.dmvae_lpips_input(p, p, 0, p, b, h, w, None) == -22 and b"lpips_input" in lib.dmvae_last_error()
    assert lib.dmvae_lpips_input(p, p, 1, p, 2 ** 31 - 1, 32768, 32768, None) == -22 and b"exceed" in lib.dmvae_last_error()


def head(lib, f, lin, ws, out, *, pairs=2, h=7, w=7, c=64, eps=1e-8, acc=0):
    return lib.dmvae_lpips_head(f, lin, pairs, h, w, c, eps, acc, ws, out, None)


def test_head_refusals(lib, p):
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert head(lib, *args) == -22 and b"NULL" in lib.dmvae_last_error()
    for kw_, needle in ((dict(pairs=0), b"pairs >= 1"), (dict(h=0), b"pairs >= 1"), (dict(w=0), b"pairs >= 1"), (dict(h=32769), b"32768"),
                        (dict(c=0), b"multiple of 4"), (dict(c=2), b"multiple of 4"), (dict(c=66), b"multiple of 4"), (dict(c=1028), b"1024"),
                        (dict(eps=0.0), b"eps"), (dict(eps=-1e-8), b"eps"), (dict(eps=float("inf")), b"eps"), (dict(eps=float("nan")), b"eps"),
                        (dict(pairs=2 ** 31, h=64, w=64), b"exceed")):
        assert head(lib, p, p, p, p, **kw_) == -22, kw_
        assert needle in lib.dmvae_last_error(), (kw_, lib.dmvae_last_error())


def closed_form(pairs, h, w, c):
    if pairs < 1 or h < 1 or w < 1 or h > 32768 or w > 32768 or c < 4 or c % 4 or c > 1024:
        return 0
    q, lanes = c // 4, 1
    while lanes < q and lanes < 64:
        lanes *= 2
    gpb = 256 // lanes
    ppb = gpb * max(1, 32768 // (8 * c) // gpb)
    nb = -(-(h * w) // ppb)
    return 0 if pairs * nb > 2 ** 31 - 1 else pairs * nb * 8


def test_workspace_closed_form(lib):
    cases = [(3, 15, 15, 64), (2, 7, 7, 192), (2, 5, 3, 384), (1, 1, 1, 256), (70, 3, 11, 64), (2, 4, 4, 1024), (128, 63, 63, 64), (1, 31, 31, 192),
             (5, 1, 1, 4), (1, 300, 200, 8), (1, 32768, 32768, 1024), (2 ** 31 - 1, 1, 1, 64), (2 ** 31, 1, 1, 64), (4, 32768, 32768, 1024),
             (0, 7, 7, 64), (1, 0, 7, 64), (1, 7, 7, 6), (1, 7, 7, 1028), (1, 7, 32769, 64)]
    for pairs, h, w, c in cases:
        assert lib.dmvae_lpips_head_workspace(pairs, h, w, c) == closed_form(pairs, h, w, c), (pairs, h, w, c)
    assert closed_form(3, 15, 15, 64) == 3 * 4 * 8 and closed_form(1, 1, 1, 256) == 8 and closed_form(2, 4, 4, 1024) == 2 * 4 * 8
    assert closed_form(2 ** 31, 1, 1, 64) == 0 and closed_form(1, 7, 7, 1028) == 0
