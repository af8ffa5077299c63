"""CPU: the device-side input pipeline's arithmetic and host logic (dmvae_amd/data.py, the host table builder of csrc/data.hip).

Three things are pinned to each other: PIL's Image.resize(LANCZOS) (where PIL is present), the numpy restatement tests/data_spec.py, and the library's
table builder; tests/golden/data_pil_lanczos.npz carries PIL's bytes to the machine that runs the kernel (tests/test_gpu_data.py)."""
import ctypes

import numpy as np
import pytest
import torch

import data_spec as D
from conftest import load_golden

# (H, W) -> Resize(384): up-scales, 8 x down-scales, pass-through, one axis untouched, a 7 x 5 source
SHAPES = [(375, 500), (500, 333), (64, 48), (7, 5), (1200, 1600), (384, 384), (384, 700), (100, 384), (97, 211), (2000, 300)]
MID = 384


def _source(h, w, seed, stripes):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if stripes:                      # rows and columns of 0 / 255: the negative lobes overshoot into the clamp at both ends
        a[::3] = 255
        a[1::3] = 0
        a[:, ::7] = 255
        a[:, 3::7] = 0
    return a


@pytest.mark.parametrize("h,w", SHAPES)
def test_spec_resize_equals_pil(h, w):
    Image = pytest.importorskip("PIL.Image")
    ow, oh = D.resized_size(w, h, MID)
    for stripes in (False, True):
        a = _source(h, w, h * 10007 + w, stripes)
        ref = np.asarray(Image.fromarray(a).resize((ow, oh), Image.LANCZOS))
        got = D.resize(a, ow, oh)
        assert got.shape == ref.shape
        assert int((got != ref).sum()) == 0, f"{h} x {w} -> {oh} x {ow}, stripes {stripes}: {int((got != ref).sum())} of {ref.size} bytes differ from PIL"


def test_spec_window_equals_crop_of_full_resize():
    a = _source(97, 211, 5, True)
    ow, oh = D.resized_size(211, 97, 48)
    full = D.resize(a, ow, oh)
    for top, left in ((0, 0), (oh - 32, ow - 32), (7, 33)):
        assert np.array_equal(D.resize(a, ow, oh, window=(top, left, 32)), full[top:top + 32, left:left + 32])


@pytest.mark.parametrize("h,w", SHAPES)
def test_library_tables_equal_spec(h, w):
    from dmvae_amd import ops
    ow, oh = D.resized_size(w, h, MID)
    for n_in, n_out in ((w, ow), (h, oh)):
        assert ops.lanczos_kmax(n_in, n_out) == D.kmax(n_in, n_out)
        # the whole axis, a window at the first border, one at the last, one inside, a single entry
        for first, count in ((0, n_out), (0, min(256, n_out)), (n_out - min(256, n_out), min(256, n_out)), (n_out // 3, min(5, n_out - n_out // 3)),
                             (n_out - 1, 1)):
            lo, n, k = ops.lanczos_table(n_in, n_out, first, count)
            slo, sn, sk = D.coeffs(n_in, n_out, first, count)
            assert lo.dtype == n.dtype == k.dtype == torch.int32 and tuple(k.shape) == sk.shape
            assert np.array_equal(lo.numpy(), slo) and np.array_equal(n.numpy(), sn), (n_in, n_out, first, count)
            assert np.array_equal(k.numpy(), sk), (n_in, n_out, first, count)
    # a wider row pitch than needed: the tail stays zero
    lo, n, k = ops.lanczos_table(w, ow, 0, 3, kmax=D.kmax(w, ow) + 5)
    assert np.array_equal(k.numpy()[:, :D.kmax(w, ow)], D.coeffs(w, ow, 0, 3)[2]) and not k[:, D.kmax(w, ow):].any()


def test_library_table_rejects():
    from dmvae_amd import _lib
    lib = _lib.lib()
    km = lib.dmvae_lanczos_kmax(500, 384)
    assert km == 2 * int(np.ceil(3.0 * 500 / 384)) + 1
    lo = (ctypes.c_int32 * 8)()
    n = (ctypes.c_int32 * 8)()
    k = (ctypes.c_int32 * (8 * km))()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert lib.dmvae_lanczos_table(500, 384, 0, 8, km, P(lo), P(n), P(k)) == 0
    assert lib.dmvae_lanczos_table(500, 384, 0, 0, km, P(lo), P(n), P(k)) == -22              # count = 0
    assert lib.dmvae_lanczos_table(500, 384, 380, 8, km, P(lo), P(n), P(k)) == -22            # first + count > out
    assert b"outside" in lib.dmvae_last_error()
    assert lib.dmvae_lanczos_table(500, 384, -1, 8, km, P(lo), P(n), P(k)) == -22
    assert lib.dmvae_lanczos_table(500, 384, 0, 8, km, None, P(n), P(k)) == -22                # NULL pointers, each
    assert lib.dmvae_lanczos_table(500, 384, 0, 8, km, P(lo), None, P(k)) == -22
    assert lib.dmvae_lanczos_table(500, 384, 0, 8, km, P(lo), P(n), None) == -22
    assert lib.dmvae_lanczos_table(500, 384, 0, 8, km - 1, P(lo), P(n), P(k)) == -22          # a short kmax
    assert b"kmax" in lib.dmvae_last_error()
    assert lib.dmvae_lanczos_table(0, 384, 0, 8, km, P(lo), P(n), P(k)) == -22
    assert lib.dmvae_lanczos_kmax(0, 5) == -22 and lib.dmvae_lanczos_kmax(5, 0) == -22
    assert lib.dmvae_lanczos_table(500, 384, 376, 8, km, P(lo), P(n), P(k)) == 0              # a window that ends at the border
    assert lo[7] + n[7] == 500
    # image_preprocess: the checks made before any launch
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.dmvae_image_preprocess(None, p, p, 1, 32, p, 0, None) == -22
    assert lib.dmvae_image_preprocess(p, p, p, 0, 32, p, 0, None) == -22
    assert lib.dmvae_image_preprocess(p, p, p, 1, 0, p, 0, None) == -22
    assert lib.dmvae_image_preprocess(p, p, p, 1, 32, p, 2, None) == -22
    assert lib.dmvae_abi_version() == 9


def test_golden_equals_spec():
    g = load_golden("data_pil_lanczos")
    mid, size = int(g["mid"]), int(g["size"])
    n_src = sum(1 for k in g if k.startswith("src_"))
    assert n_src >= 5
    for i in range(n_src):
        src, par, out = g[f"src_{i}"], g[f"par_{i}"], g[f"out_{i}"]
        assert src.dtype == np.uint8 and out.shape == (len(par), size, size, 3)
        for (flip, top, left), ref in zip(par.tolist(), out):
            assert np.array_equal(D.pipeline(src, mid, size, flip, top, left), ref), (i, src.shape, flip, top, left)


def test_golden_equals_pil():
    Image = pytest.importorskip("PIL.Image")
    g = load_golden("data_pil_lanczos")
    mid, size = int(g["mid"]), int(g["size"])
    for i in range(sum(1 for k in g if k.startswith("src_"))):
        src = g[f"src_{i}"]
        for (flip, top, left), ref in zip(g[f"par_{i}"].tolist(), g[f"out_{i}"]):
            img = Image.fromarray(src[:, ::-1].copy() if flip else src)
            ow, oh = D.resized_size(img.size[0], img.size[1], mid)
            img = img.resize((ow, oh), Image.LANCZOS)
            assert np.array_equal(np.asarray(img)[top:top + size, left:left + size], ref), (i, flip, top, left)


# ---- host logic -----------------------------------------------------------------------------------------------------------------------
def test_size_rule():
    from dmvae_amd.data import resized_size
    assert resized_size(500, 375, 384) == (512, 384)
    assert resized_size(333, 500, 384) == (384, 576)
    assert resized_size(300, 2000, 384) == (384, 2560)
    assert resized_size(5, 7, 384) == (384, 537)                     # int(), not round(): 384 * 7 / 5 = 537.6
    assert resized_size(384, 384, 384) == (384, 384)
    assert resized_size(700, 384, 384) == (700, 384)                 # the pass-through: the shorter edge already is mid
    assert resized_size(384, 100, 384) == (1474, 384)
    for w, h in ((500, 375), (97, 211), (48, 48), (1000, 33)):
        assert resized_size(w, h, 48) == D.resized_size(w, h, 48)
    with pytest.raises(ValueError):
        resized_size(0, 5, 48)


def test_center_offsets_round_half_to_even():
    from dmvae_amd.data import center_crop_offsets
    assert center_crop_offsets(384, 512, 256) == (64, 128)           # even slack
    assert center_crop_offsets(257, 259, 256) == (0, 2)              # slack 1 -> round(0.5) = 0, slack 3 -> round(1.5) = 2: Python's round
    assert center_crop_offsets(261, 263, 256) == (2, 4)              # slack 5 -> round(2.5) = 2, slack 7 -> round(3.5) = 4
    assert center_crop_offsets(256, 256, 256) == (0, 0)
    with pytest.raises(ValueError):
        center_crop_offsets(255, 300, 256)


def test_draw_order_and_single_value_ranges(monkeypatch):
    from dmvae_amd.data import DeviceInputPipeline, RaggedImages
    # (H, W) -> mid 48: (64, 48) resizes to itself in W: H' = 64, W' = 48; (48, 48) has both ranges single-valued; (60, 90) -> 48 x 72
    sizes = [(64, 48), (48, 48), (60, 90), (96, 48)]
    meta = torch.tensor([[0, h, w] for h, w in sizes], dtype=torch.int64)
    ragged = RaggedImages(torch.zeros(3 * 96 * 90, dtype=torch.uint8), meta)
    calls = []
    real_rand, real_randint = torch.rand, torch.randint

    def rand(*a, **k):
        calls.append(("rand",))
        return real_rand(*a, **k)

    def randint(lo, hi, *a, **k):
        calls.append(("randint", lo, hi))
        return real_randint(lo, hi, *a, **k)

    monkeypatch.setattr(torch, "rand", rand)
    monkeypatch.setattr(torch, "randint", randint)
    pipe = DeviceInputPipeline(image_size=48, mid_reso=1.0, mode="train", hflip=True, generator=torch.Generator().manual_seed(3))
    assert pipe.sizes(ragged) == [(64, 48), (48, 48), (48, 72), (96, 48)]
    flip, top, left = pipe.draw(ragged)
    assert calls == [("rand",), ("randint", 0, 17), ("rand",), ("rand",), ("randint", 0, 25), ("rand",), ("randint", 0, 49)]
    # the same generator state replayed by hand, in the stated order
    g = torch.Generator().manual_seed(3)
    exp_flip, exp_top, exp_left = [0] * 4, [0] * 4, [0] * 4
    exp_flip[0] = int(real_rand(1, generator=g).item() < 0.5)
    exp_top[0] = real_randint(0, 17, (1,), generator=g).item()
    exp_flip[1] = int(real_rand(1, generator=g).item() < 0.5)
    exp_flip[2] = int(real_rand(1, generator=g).item() < 0.5)
    exp_left[2] = real_randint(0, 25, (1,), generator=g).item()
    exp_flip[3] = int(real_rand(1, generator=g).item() < 0.5)
    exp_top[3] = real_randint(0, 49, (1,), generator=g).item()
    assert flip.tolist() == exp_flip and top.tolist() == exp_top and left.tolist() == exp_left
    # hflip off: no flip draw; val mode: no draw at all, centre offsets
    calls.clear()
    f2, _, _ = DeviceInputPipeline(48, 1.0, "train", hflip=False, generator=torch.Generator().manual_seed(3)).draw(ragged)
    assert [c[0] for c in calls] == ["randint"] * 3 and f2.tolist() == [0] * 4
    calls.clear()
    f3, t3, l3 = DeviceInputPipeline(48, 1.0, "val").draw(ragged)
    assert calls == [] and f3.tolist() == [0] * 4 and t3.tolist() == [8, 0, 0, 24] and l3.tolist() == [0, 0, 12, 0]


def test_pack_images_offsets_pinning_rejects():
    from dmvae_amd.data import RaggedImages, collate_ragged, pack_images
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (7, 5, 3), dtype=np.uint8)
    b = torch.from_numpy(rng.integers(0, 256, (4, 9, 3), dtype=np.uint8))
    c = rng.integers(0, 256, (6, 6, 3), dtype=np.uint8)[:, ::2]          # a non-contiguous view
    r = pack_images([a, b, c])
    assert isinstance(r, RaggedImages) and len(r) == 3
    assert r.meta.tolist() == [[0, 7, 5], [105, 4, 9], [213, 6, 3]] and r.data.numel() == 213 + 54 and r.data.dtype == torch.uint8
    assert np.array_equal(r.image(0).numpy(), a) and torch.equal(r.image(1), b) and np.array_equal(r.image(2).numpy(), c)
    assert r.data.is_pinned() == torch.cuda.is_available()
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        rp = pack_images([Image.fromarray(a), b])
        assert np.array_equal(rp.image(0).numpy(), a) and rp.meta.tolist() == [[0, 7, 5], [105, 4, 9]]
        with pytest.raises(ValueError):
            pack_images([Image.fromarray(a).convert("L")])
    for bad in ([], [a.astype(np.float32)], [a[:, :, :2]], [a[0]], [np.zeros((0, 5, 3), np.uint8)], [b.float()], ["x.png"], [b.permute(2, 0, 1)]):
        with pytest.raises(ValueError):
            pack_images(bad)
    with pytest.raises(ValueError):
        RaggedImages(torch.zeros(10, dtype=torch.uint8), torch.tensor([[0, 2, 2]]))      # 12 bytes do not fit in 10
    ragged, labels = collate_ragged([(a, 3), (b, 1)])
    assert len(ragged) == 2 and labels.tolist() == [3, 1] and labels.dtype == torch.int64


def test_tables_records_and_rejects():
    from dmvae_amd import _lib
    from dmvae_amd.data import DeviceInputPipeline, pack_images
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((7, 5), (48, 90), (90, 48), (48, 48), (100, 75))]
    ragged = pack_images(imgs)
    pipe = DeviceInputPipeline(image_size=32, mid_reso=1.5, mode="val")
    flip, top, left = pipe.draw(ragged)
    rec, taps = pipe.tables(ragged, flip, top, left)
    assert tuple(rec.shape) == (5, _lib.IMAGE_RECORD_WORDS) and rec.dtype == torch.int64 and taps.dtype == torch.int32
    assert rec[:, :3].tolist() == ragged.meta.tolist()
    assert rec[:, 3:5].tolist() == [[67, 48], [48, 90], [90, 48], [48, 48], [64, 48]]
    assert rec[1, 9] == -1 and rec[1, 8] == -1 and rec[2, 8] == -1 and rec[2, 9] == -1 and rec[3, 8] == -1 and rec[3, 9] == -1   # pass-through images
    # image 0: x table then y table, each lo[S], n[S], k[S][kmax], equal to the spec's window
    xo, yo, kmx, kmy = rec[0, 8:12].tolist()
    assert (xo, kmx, kmy) == (0, 7, 7) and yo == 2 * 32 + 32 * 7
    slo, sn, sk = D.coeffs(5, 48, int(left[0]), 32)
    assert np.array_equal(taps[:32].numpy(), slo) and np.array_equal(taps[32:64].numpy(), sn) and np.array_equal(taps[64:64 + 224].numpy(), sk.reshape(-1))
    slo, sn, sk = D.coeffs(7, 67, int(top[0]), 32)
    assert np.array_equal(taps[yo:yo + 32].numpy(), slo) and np.array_equal(taps[yo + 64:yo + 64 + 224].numpy(), sk.reshape(-1))
    with pytest.raises(ValueError):
        pipe.tables(ragged, flip, top + 100, left)
    with pytest.raises(ValueError):
        pipe.tables(ragged, flip[:2], top, left)
    with pytest.raises(ValueError):
        pipe.tables(ragged, flip + 2, top, left)
    with pytest.raises(_lib.DmvaeHipError):
        pipe.apply(ragged, flip, top, left)                              # the pack is on the host: there is no CPU path
    with pytest.raises(ValueError):
        DeviceInputPipeline(mode="test")


class _ArrayDataset(torch.utils.data.Dataset):
    """Decoded images of different sizes, as a decode-only DatasetFolder yields them: (uint8 [H, W, 3], label)."""
    SIZES = [(7, 5), (12, 9), (6, 6), (5, 11), (9, 4), (8, 8)]

    def __len__(self):
        return len(self.SIZES)

    def __getitem__(self, i):
        h, w = self.SIZES[i]
        return np.random.default_rng(i).integers(0, 256, (h, w, 3), dtype=np.uint8), i


def _collate_watching_the_worker(samples):
    """collate_ragged inside a worker in which any question to the GPU runtime and any request for pinned memory raises."""
    from dmvae_amd.data import collate_ragged
    assert torch.utils.data.get_worker_info() is not None

    def forbidden(*a, **k):
        raise AssertionError("a DataLoader worker asked the GPU runtime")

    real_empty, real_pin = torch.empty, torch.Tensor.pin_memory

    def empty(*a, **k):
        assert not k.get("pin_memory"), "a DataLoader worker asked for pinned memory"
        return real_empty(*a, **k)

    torch.cuda.is_available = torch.cuda.device_count = torch.cuda.init = torch.cuda._lazy_init = forbidden
    torch.Tensor.pin_memory = forbidden
    torch.empty = empty
    try:
        return collate_ragged(samples)
    finally:
        torch.empty, torch.Tensor.pin_memory = real_empty, real_pin


def test_collate_ragged_behind_dataloader_workers():
    """The documented wiring: collate_ragged runs inside the worker processes.  Nothing there pins or asks for the GPU; the pack that arrives is whole, and
    RaggedImages has the pin_memory() the loader's pin thread looks for."""
    from dmvae_amd.data import RaggedImages
    ds = _ArrayDataset()
    loader = torch.utils.data.DataLoader(ds, batch_size=3, num_workers=2, collate_fn=_collate_watching_the_worker)
    seen = 0
    for ragged, labels in loader:
        assert isinstance(ragged, RaggedImages) and len(ragged) == 3 and labels.dtype == torch.int64
        assert not ragged.is_pinned()
        for j, lab in enumerate(labels.tolist()):
            assert np.array_equal(ragged.image(j).numpy(), ds[lab][0])
        seen += len(ragged)
    assert seen == len(ds)
    assert callable(getattr(RaggedImages, "pin_memory", None))
    if torch.cuda.is_available():
        pinned = ragged.pin_memory()
        assert pinned.is_pinned() and pinned.pin_memory() is pinned and torch.equal(pinned.data, ragged.data) and pinned.meta is ragged.meta
