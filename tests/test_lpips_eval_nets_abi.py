"""CPU: the two entry points the evaluation LPIPS' 'vgg' and 'squeeze' networks add -- dmvae_maxpool2d_f32 (csrc/inception.hip) and dmvae_lpips_head_form
(csrc/lpips_eval.hip) -- are declared, exported and bound at ABI version 9, and refuse everything outside their contract with -22 and a message naming the
entry before any launch (no GPU is touched: every call below returns from argument validation, and the buffers handed in keep their bytes).  VGG's first
layer, cin 3 with a (3, 3) padding 1 kernel, and the Fire modules' forms pass dmvae_conv2d_f32_fwd's form, channel and size checks."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

ENTRY_POINTS = ("dmvae_maxpool2d_f32", "dmvae_lpips_head_form")
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    from dmvae_amd import _lib
    return _lib.lib()


@pytest.fixture
def bufs():
    """Two host buffers with a known fill: a refusing entry neither launches nor writes."""
    raw = [ctypes.create_string_buffer(bytes([FILL]) * 256, 256) for _ in range(2)]
    yield raw, [ctypes.cast(b, ctypes.c_void_p) for b in raw]
    assert all(b.raw == bytes([FILL]) * 256 for b in raw)


def test_entry_points_are_declared_exported_and_bound(lib):
    from dmvae_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmvae_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} is not declared in include/dmvae_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["dmvae_lpips_head_form"][1]) == len(_lib.SIGNATURES["dmvae_lpips_head"][1]) + 1      # one more argument: form
    assert lib.dmvae_abi_version() == 9 and _lib.ABI_VERSION == 9                     # additions only
    assert callable(ops.maxpool2d_f32) and "form" in ops.lpips_head.__code__.co_varnames


def pool(lib, x, y, *, batch=2, h=8, w=8, c=16, kernel=2, stride=2, ceil=0, off=0, pitch=None):
    return lib.dmvae_maxpool2d_f32(x, y, batch, h, w, c, kernel, stride, ceil, off, c if pitch is None else pitch, None)


@pytest.mark.parametrize("kw_,needle", [
    (dict(kernel=2, stride=2, ceil=1), b"not built"),
    (dict(kernel=3, stride=2, ceil=0), b"not built"),
    (dict(kernel=3, stride=1, ceil=1), b"not built"),
    (dict(kernel=2, stride=1), b"not built"),
    (dict(kernel=4, stride=2), b"not built"),
    (dict(kernel=0, stride=2), b"not built"),
    (dict(h=1), b"h, w >= 2"),
    (dict(w=1), b"h, w >= 2"),
    (dict(kernel=3, ceil=1, h=2), b"h, w >= 3"),
    (dict(kernel=3, ceil=1, w=2), b"h, w >= 3"),
    (dict(batch=0), b"batch >= 1"),
    (dict(h=0), b"batch >= 1"),
    (dict(w=40000), b"32768"),
    (dict(c=0), b"multiple of 4"),
    (dict(c=6), b"multiple of 4"),
    (dict(c=16, off=4, pitch=16), b"do not fit"),
    (dict(c=16, off=2, pitch=32), b"do not fit"),
    (dict(c=16, off=0, pitch=18), b"do not fit"),
    (dict(c=16, off=-4, pitch=32), b"do not fit"),
    (dict(batch=2 ** 31 - 1, h=32768, w=32768, c=16), b"exceed"),
    (dict(kernel=3, ceil=1, batch=2 ** 31 - 1, h=32768, w=32768, c=2 ** 31 - 4, pitch=2 ** 31 - 4), b"exceed"),
    (dict(batch=2 ** 17, h=256, w=256, c=1024), b"exceed"),
])
def test_maxpool_refusals(lib, bufs, kw_, needle):
    _, (x, y) = bufs
    assert pool(lib, x, y, **kw_) == -22, kw_
    msg = lib.dmvae_last_error()
    assert msg.startswith(b"maxpool2d_f32:") and needle in msg, (kw_, msg)


def test_maxpool_null_pointers(lib, bufs):
    _, (x, y) = bufs
    for args in ((None, y), (x, None)):
        assert pool(lib, *args) == -22 and lib.dmvae_last_error().startswith(b"maxpool2d_f32: NULL")


def test_pool2d_f32_keeps_its_three_modes(lib, bufs):
    """The new pools are a new entry: dmvae_pool2d_f32 still refuses every mode past 2."""
    _, (x, y) = bufs
    for mode in (3, 4, -1):
        assert lib.dmvae_pool2d_f32(x, y, mode, 1, 8, 8, 16, 0, 16, None) == -22 and b"mode" in lib.dmvae_last_error()


def head(lib, f, lin, ws, out, *, pairs=2, h=7, w=7, c=64, eps=1e-10, form=1, acc=0):
    return lib.dmvae_lpips_head_form(f, lin, pairs, h, w, c, eps, form, acc, ws, out, None)


def test_head_form_refusals(lib, bufs):
    _, (p, q) = bufs
    for args in ((None, p, p, q), (p, None, p, q), (p, p, None, q), (p, p, p, None)):
        assert head(lib, *args) == -22 and lib.dmvae_last_error().startswith(b"lpips_head_form: NULL")
    for form in (0, 1):
        for kw_, needle in ((dict(pairs=0), b"pairs >= 1"), (dict(h=0), b"pairs >= 1"), (dict(w=0), b"pairs >= 1"), (dict(h=32769), b"32768"),
                            (dict(c=0), b"multiple of 4"), (dict(c=2), b"multiple of 4"), (dict(c=66), b"multiple of 4"), (dict(c=1028), b"1024"),
                            (dict(eps=0.0), b"eps"), (dict(eps=-1e-8), b"eps"), (dict(eps=float("inf")), b"eps"), (dict(eps=float("nan")), b"eps"),
                            (dict(pairs=2 ** 31, h=64, w=64), b"exceed")):
            assert head(lib, p, p, p, q, form=form, **kw_) == -22, kw_
            msg = lib.dmvae_last_error()
            assert msg.startswith(b"lpips_head_form:") and needle in msg, (kw_, msg)
    for form in (2, -1, 7):
        assert head(lib, p, p, p, q, form=form) == -22
        assert lib.dmvae_last_error().startswith(b"lpips_head_form: form must be 0")
    # the older entry keeps its own name in its messages
    assert lib.dmvae_lpips_head(p, p, 0, 7, 7, 64, 1e-8, 0, p, q, None) == -22 and lib.dmvae_last_error().startswith(b"lpips_head: pairs")


def test_conv_validation_takes_vgg_first_layer_and_the_fire_forms(lib, bufs):
    """cin 3 with a (3, 3) padding (1, 1) kernel (VGG's conv1_1), cin 3 (3, 3) stride 2 padding 0 (SqueezeNet's features[0]) and the Fire modules' channel
    counts pass the form, channel and size checks of dmvae_conv2d_f32_fwd: handed a channel slice that does not fit -- the last argument check before the
    launch -- the slice is what the entry complains about.  (That the forms compute is tests/test_gpu_lpips_eval_nets.py's business.)"""
    _, (p, q) = bufs
    forms = [(3, 64, 3, 1, 1), (3, 64, 3, 2, 0), (64, 16, 1, 1, 0), (16, 64, 3, 1, 1), (48, 192, 1, 1, 0), (48, 192, 3, 1, 1), (512, 64, 1, 1, 0),
             (64, 256, 3, 1, 1), (512, 512, 3, 1, 1)]
    for cin, cout, k, stride, pad in forms:
        assert lib.dmvae_conv2d_f32_fwd(p, p, None, p, q, 1, 16, 16, cin, cout, k, k, stride, pad, pad, 1, 4, cout, None) == -22
        assert b"do not fit" in lib.dmvae_last_error(), (cin, cout, k, lib.dmvae_last_error())
    assert lib.dmvae_conv2d_f32_fwd(p, p, None, p, q, 1, 16, 16, 3, 64, 3, 3, 1, 2, 2, 1, 4, 64, None) == -22 and b"not built" in lib.dmvae_last_error()
