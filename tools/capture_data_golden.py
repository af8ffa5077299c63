#!/usr/bin/env python3
"""Record tests/golden/data_pil_lanczos.npz: a few small decoded sources and PIL's own bytes for flip -> Resize(mid, LANCZOS) -> crop on them, so that a
machine without PIL can hold csrc/data.hip to PIL bit for bit (tests/test_gpu_data.py) and the numpy restatement (tests/data_spec.py) is pinned three ways
(tests/test_data_cpu.py).  Needs PIL; neither torch nor a GPU.

    python tools/capture_data_golden.py [--out tests/golden/data_pil_lanczos.npz]

Keys: `mid`, `size` (the Resize edge and the crop), `pil_version`; per case i: `src_i` uint8 [H, W, 3], `par_i` int64 [n, 3] rows of (flip, top, left),
`out_i` uint8 [n, size, size, 3]."""
import argparse
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MID, SIZE = 48, 32
# (H, W): up-scale with taps clipped at both borders; ~2 x down; one pass skipped either way; both skipped; odd widths; stripes into the clamp
SHAPES = [(7, 5), (100, 75), (48, 90), (90, 48), (48, 48), (49, 47), (61, 130)]


def resized_size(w, h, mid):
    """torchvision's Resize(int) rule, restated (torchvision is not needed here)."""
    short, long = (w, h) if w <= h else (h, w)
    if short == mid:
        return w, h
    new_long = int(mid * long / short)
    return (mid, new_long) if w <= h else (new_long, mid)


def pil_pipeline(src, flip, top, left):
    img = Image.fromarray(src)
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)                  # what torchvision's hflip does to a PIL image
    ow, oh = resized_size(img.size[0], img.size[1], MID)
    if (ow, oh) != img.size:
        img = img.resize((ow, oh), Image.LANCZOS)
    return np.asarray(img.crop((left, top, left + SIZE, top + SIZE)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "data_pil_lanczos.npz"))
    args = ap.parse_args()
    rng = np.random.default_rng(20)
    rec = {"mid": np.int64(MID), "size": np.int64(SIZE), "pil_version": np.array(PIL.__version__)}
    for i, (h, w) in enumerate(SHAPES):
        src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i % 2:                                                   # stripes of 0 / 255: the negative lobes reach the clamp at both ends
            src[::3] = 255
            src[1::3] = 0
            src[:, ::5] = 0
        ow, oh = resized_size(w, h, MID)
        my, mx = oh - SIZE, ow - SIZE
        par = np.array([[0, 0, 0], [1, my, mx], [1, int(rng.integers(0, my + 1)), int(rng.integers(0, mx + 1))],
                        [0, int(round(my / 2.0)), int(round(mx / 2.0))]], dtype=np.int64)
        rec[f"src_{i}"] = src
        rec[f"par_{i}"] = par
        rec[f"out_{i}"] = np.stack([pil_pipeline(src, *p) for p in par.tolist()])
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {len(SHAPES)} sources, {os.path.getsize(args.out)} bytes, PIL {PIL.__version__}", file=sys.stderr)


if __name__ == "__main__":
    main()
