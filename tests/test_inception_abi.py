"""CPU: the Inception extractor's entry points (csrc/inception.hip) are declared, exported and bound, and refuse everything outside their forms with -22 and
a message before any launch (no GPU is touched: every call below returns from argument validation)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

ENTRY_POINTS = ("dmvae_conv2d_f32_fwd", "dmvae_pool2d_f32", "dmvae_global_avgpool_f32", "dmvae_inception_input")


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
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.dmvae_abi_version() == 9 and _lib.ABI_VERSION == 9                     # additions only
    for fn in ("conv2d_f32", "pool2d_f32", "global_avgpool_f32", "inception_input", "pack_conv_weight_f32"):
        assert callable(getattr(ops, fn))


def conv(lib, x, w, y, *, b=2, h=9, wd=11, cin=16, cout=16, kh=3, kw=3, stride=1, ph=0, pw=0, off=0, pitch=None):
    return lib.dmvae_conv2d_f32_fwd(x, w, None, None, y, b, h, wd, cin, cout, kh, kw, stride, ph, pw, 1, off, cout if pitch is None else pitch, None)


@pytest.mark.parametrize("kw_,needle", [
    (dict(kh=2, kw=2), b"(2, 2)"),                                   # a 2 x 2 kernel
    (dict(stride=3), b"stride 3"),
    (dict(cout=24), b"cout must be a multiple of 16"),
    (dict(cin=20), b"cin must be 3 or a multiple of 16"),
    (dict(kh=1, kw=7, ph=1, pw=1), b"(1, 7)"),                       # pad (1, 1) on a 1 x 7
    (dict(kh=3, kw=3, stride=2, ph=1, pw=1), b"stride 2"),           # the stride-2 form has no padding
    (dict(kh=5, kw=5, ph=0, pw=0), b"(5, 5)"),
    (dict(off=16, pitch=24), b"do not fit"),                         # out_c_offset + cout > out_c_pitch
    (dict(off=2, pitch=32), b"do not fit"),                          # an offset that is no multiple of 4
    (dict(h=2, wd=2), b"smaller than"),
    (dict(b=0), b"batch >= 1"),
])
def test_conv_refuses_what_it_does_not_build(lib, p, kw_, needle):
    assert conv(lib, p, p, p, **kw_) == -22
    assert needle in lib.dmvae_last_error(), lib.dmvae_last_error()


def test_null_pointers_are_refused(lib, p):
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert conv(lib, *args) == -22 and b"NULL" in lib.dmvae_last_error()
    for args in ((None, p), (p, None)):
        assert lib.dmvae_pool2d_f32(*args, 0, 1, 9, 11, 16, 0, 16, None) == -22 and b"NULL" in lib.dmvae_last_error()
        assert lib.dmvae_global_avgpool_f32(*args, 1, 8, 8, 16, None) == -22 and b"NULL" in lib.dmvae_last_error()
    assert lib.dmvae_inception_input(None, 1, p, 1, 8, 8, None) == -22 and b"NULL" in lib.dmvae_last_error()
    assert lib.dmvae_inception_input(p, 1, None, 1, 8, 8, None) == -22 and b"NULL" in lib.dmvae_last_error()


def test_pool_and_the_small_kernels_refuse_bad_sizes(lib, p):
    assert lib.dmvae_pool2d_f32(p, p, 3, 1, 9, 11, 16, 0, 16, None) == -22 and b"mode" in lib.dmvae_last_error()
    assert lib.dmvae_pool2d_f32(p, p, 0, 1, 2, 11, 16, 0, 16, None) == -22 and b"h, w >= 3" in lib.dmvae_last_error()
    assert lib.dmvae_pool2d_f32(p, p, 1, 1, 9, 11, 18, 0, 20, None) == -22 and b"multiple of 4" in lib.dmvae_last_error()
    assert lib.dmvae_pool2d_f32(p, p, 2, 1, 9, 11, 16, 16, 24, None) == -22 and b"do not fit" in lib.dmvae_last_error()
    assert lib.dmvae_global_avgpool_f32(p, p, 1, 0, 8, 16, None) == -22
    assert lib.dmvae_inception_input(p, 0, p, 0, 8, 8, None) == -22
