"""The arithmetic of the device-side input pipeline, restated in numpy: PIL's 8-bit LANCZOS resize (libImaging/Resample.c), torchvision's Resize(int)
size rule, flip, crop and the float conversion.  Test infrastructure only; tests/test_data_cpu.py holds `resize` to PIL byte for byte, the library's
table builder to `coeffs`, and tests/test_gpu_data.py holds the kernel to `pipeline`.

The filter argument is `(j + lo - center + 0.5) * (1.0 / fs)`, a multiplication by the reciprocal as Resample.c writes it, not a division by fs, and
lanczos3 is `sinc(x) * sinc(x / 3)` with `sinc(t) = sin(t * pi) / (t * pi)` (the division by 3 comes before the multiplication by pi).  Either can differ
from the other form in the last ulp; PIL's bytes are the yardstick."""
import math

import numpy as np

PRECISION_BITS = 22


def resized_size(w, h, mid):
    """torchvision Resize(mid): (w', h')."""
    short, long = (w, h) if w <= h else (h, w)
    if short == mid:
        return w, h
    new_long = int(mid * long / short)
    return (mid, new_long) if w <= h else (new_long, mid)


def center_crop_offsets(h, w, s):
    return int(round((h - s) / 2.0)), int(round((w - s) / 2.0))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos3(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def kmax(n_in, n_out):
    return int(math.ceil(3.0 * max(n_in / n_out, 1.0))) * 2 + 1


def coeffs(n_in, n_out, first=0, count=None):
    """-> (lo [count], n [count], k [count, kmax]) int32, the tables of output indices first .. first + count - 1."""
    count = n_out - first if count is None else count
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ss = 1.0 / fs
    km = kmax(n_in, n_out)
    lo = np.zeros(count, np.int32)
    n = np.zeros(count, np.int32)
    k = np.zeros((count, km), np.int32)
    for i in range(count):
        center = (first + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xn = min(int(center + support + 0.5), n_in) - xmin
        w = [lanczos3((j + xmin - center + 0.5) * ss) for j in range(xn)]
        ww = 0.0
        for v in w:
            ww += v
        for j, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            k[i, j] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        lo[i], n[i] = xmin, xn
    return lo, n, k


def _clip8(v):
    return np.clip(v >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _pass(a, axis_in, n_out, first, count):
    """One resampling pass along axis 1 of a [R, n_in, C] uint8 array, int32 arithmetic with int32 wrap-around (as C)."""
    lo, n, k = coeffs(axis_in, n_out, first, count)
    out = np.empty((a.shape[0], count, a.shape[2]), np.uint8)
    a64 = a.astype(np.int64)
    for i in range(count):
        kk = k[i, :n[i]].astype(np.int64)
        s = (a64[:, lo[i]:lo[i] + n[i], :] * kk[None, :, None]).sum(1) + (1 << (PRECISION_BITS - 1))
        out[:, i, :] = _clip8(s.astype(np.int32))
    return out


def resize(a, ow, oh, window=None):
    """PIL's Image.resize((ow, oh), LANCZOS) of a uint8 [H, W, C] array; window = (top, left, s) computes only that crop of the result."""
    h, w, _ = a.shape
    top, left, sh, sw = (0, 0, oh, ow) if window is None else (window[0], window[1], window[2], window[2])
    if ow != w:
        a = _pass(a, w, ow, left, sw)                      # horizontal first, rounded to uint8
    else:
        a = a[:, left:left + sw]
    if oh != h:
        a = _pass(a.transpose(1, 0, 2), h, oh, top, sh).transpose(1, 0, 2)
    else:
        a = a[top:top + sh]
    return np.ascontiguousarray(a)


def pipeline(a, mid, s, flip, top, left):
    """flip -> Resize(mid, LANCZOS) -> crop s x s at (top, left): uint8 [s, s, 3]."""
    if flip:
        a = a[:, ::-1]
    h, w, _ = a.shape
    ow, oh = resized_size(w, h, mid)
    assert 0 <= top <= oh - s and 0 <= left <= ow - s
    return resize(np.ascontiguousarray(a), ow, oh, window=(top, left, s))


def to_float(u8_nhwc):
    """ToTensor then x + x - 1 on a uint8 [B, S, S, 3] array -> float32 [B, 3, S, S]."""
    v = u8_nhwc.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)
    return (v + v) + np.float32(-1.0)
