"""The device-side input pipeline on the MI355X (-m gpu): csrc/data.hip against tests/data_spec.py (the numpy restatement that tests/test_data_cpu.py holds
to PIL byte for byte) and against PIL's own recorded bytes (tests/golden/data_pil_lanczos.npz), everything under torch.equal.

image_size = 32 with mid_reso = 1.5 (the shorter edge becomes 48) lets small sources reach every regime of the kernel."""
import warnings

import numpy as np
import pytest
import torch

import data_spec as D
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, MID = 32, 48
GUARD = 0xA5
# (H, W): up-scale with taps clipped at both borders; ~6 x down, ~37 taps; vertical pass skipped; horizontal pass skipped; both skipped (pure crop); one
# axis ~21 x down and the other up; widths that are no multiple of 4 bytes
SHAPES = [(7, 5), (400, 300), (48, 90), (90, 48), (48, 48), (33, 1000), (49, 47)]


def _sources():
    rng = np.random.default_rng(11)
    out = []
    for i, (h, w) in enumerate(SHAPES):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i in (1, 5):                  # stripes of 0 / 255 on the down-scaled sources: the negative lobes reach the clamp
            a[::5] = 255
            a[2::5] = 0
            a[:, ::9] = 0
            a[:, 4::9] = 255
        out.append(a)
    return out


SOURCES = _sources()


def _pack(sources, order=None):
    """A hand-made pack: guard bytes of odd lengths in front of, between and after the images, so that every image starts at an unaligned offset."""
    from dmvae_amd.data import RaggedImages
    order = list(range(len(sources))) if order is None else order
    chunks, meta, off = [], [], 0
    for j, i in enumerate(order):
        g = 1 + 2 * (j % 4)
        chunks.append(np.full(g, GUARD, np.uint8))
        off += g
        a = sources[i]
        meta.append([off, a.shape[0], a.shape[1]])
        chunks.append(a.reshape(-1))
        off += a.size
    chunks.append(np.full(13, GUARD, np.uint8))
    host = torch.from_numpy(np.concatenate(chunks))
    mask = torch.ones(host.numel(), dtype=torch.bool)
    for o, h, w in meta:
        mask[o:o + 3 * h * w] = False
    return RaggedImages(host, torch.tensor(meta, dtype=torch.int64)), mask


def _pipe(size=S, mid_reso=1.5, **kw):
    from dmvae_amd.data import DeviceInputPipeline
    return DeviceInputPipeline(image_size=size, mid_reso=mid_reso, **kw)


_SPEC = {}


def _spec(i, flip, top, left, sources=SOURCES, mid=MID, size=S, tag="batch"):
    """The spec's bytes of one image, computed once per (source set, image, draw) and shared."""
    key = (tag, i, flip, top, left, mid, size)
    if key not in _SPEC:
        _SPEC[key] = torch.from_numpy(D.pipeline(sources[i], mid, size, flip, top, left))
    return _SPEC[key]


def _draws(pipe, ragged, flips, crops):
    b = len(ragged)
    sizes = pipe.sizes(ragged)
    g = torch.Generator().manual_seed(7)
    flip = {"off": torch.zeros(b, dtype=torch.int64), "on": torch.ones(b, dtype=torch.int64), "mixed": torch.arange(b) % 2}[flips]
    if crops == "zero":
        top, left = torch.zeros(b, dtype=torch.int64), torch.zeros(b, dtype=torch.int64)
    elif crops == "max":
        top = torch.tensor([h2 - pipe.image_size for h2, _ in sizes])
        left = torch.tensor([w2 - pipe.image_size for _, w2 in sizes])
    else:
        top = torch.tensor([int(torch.randint(0, h2 - pipe.image_size + 1, (1,), generator=g)) for h2, _ in sizes])
        left = torch.tensor([int(torch.randint(0, w2 - pipe.image_size + 1, (1,), generator=g)) for _, w2 in sizes])
    return flip, top, left


@pytest.mark.parametrize("crops", ["zero", "max", "drawn"])
@pytest.mark.parametrize("flips", ["off", "on", "mixed"])
def test_u8_equals_spec_with_guards(flips, crops):
    """The ragged batch under each flip / crop setting: equal to the spec under torch.equal; the 0xA5 bytes around the images and the sentinel rows around
    the output intact; a second call gives the same bytes."""
    pipe = _pipe()
    ragged, mask = _pack(SOURCES)
    flip, top, left = _draws(pipe, ragged, flips, crops)
    dev = ragged.to(DEV)
    b = len(ragged)
    row = S * 3
    buf = torch.full((row + b * S * row + row,), 0x5C, dtype=torch.uint8, device=DEV)
    into = buf[row:row + b * S * row].view(b, S, S, 3)
    got = pipe.apply(dev, flip, top, left, out="u8", into=into)
    assert got.data_ptr() == into.data_ptr()
    want = torch.stack([_spec(i, int(flip[i]), int(top[i]), int(left[i])) for i in range(b)])
    got_h = got.cpu()
    for i in range(b):
        assert torch.equal(got_h[i], want[i]), f"image {i} {SHAPES[i]} flip {int(flip[i])} crop ({int(top[i])}, {int(left[i])}): " \
                                               f"{int((got_h[i] != want[i]).sum())} bytes differ"
    assert bool((buf[:row] == 0x5C).all()) and bool((buf[-row:] == 0x5C).all())
    back = dev.data.cpu()
    assert torch.equal(back, ragged.data) and bool((back[mask] == GUARD).all())
    again = pipe.apply(dev, flip, top, left, out="u8")
    assert torch.equal(again, got)


def test_position_in_the_pack_does_not_matter():
    """B = 1 for every image, and the batch in reverse order with other guard lengths: the same per-image bytes."""
    pipe = _pipe()
    ragged, _ = _pack(SOURCES)
    flip, top, left = _draws(pipe, ragged, "mixed", "drawn")
    base = pipe.apply(ragged.to(DEV), flip, top, left, out="u8")
    order = list(range(len(SOURCES)))[::-1][:5]
    rev, _ = _pack(SOURCES, order)
    idx = torch.tensor(order)
    got = pipe.apply(rev.to(DEV), flip[idx], top[idx], left[idx], out="u8")
    assert got.shape[0] == 5 and torch.equal(got, base[idx.to(DEV)])
    for i in range(len(SOURCES)):
        one, _ = _pack(SOURCES, [i])
        got1 = pipe.apply(one.to(DEV), flip[i:i + 1], top[i:i + 1], left[i:i + 1], out="u8")
        assert torch.equal(got1[0], base[i]), i


def _to_float_host(u8):
    """ToTensor and normalize_01_into_pm1 as the reference's workers run them: on the HOST, where `.div(255)` is a true IEEE division.  (On a GPU tensor
    torch divides by a Python scalar as a multiplication by 1 / 255 in f32, which rounds about half of the 256 byte values differently; the reference never
    does that, so the expectation is formed on the host.)"""
    x = u8.cpu().permute(0, 3, 1, 2).float().div(255)
    return x.add(x).add_(-1)


def test_f32_is_totensor_then_x_plus_x_minus_one():
    pipe = _pipe()
    ragged, _ = _pack(SOURCES)
    flip, top, left = _draws(pipe, ragged, "mixed", "drawn")
    dev = ragged.to(DEV)
    u8 = pipe.apply(dev, flip, top, left, out="u8")
    f = pipe.apply(dev, flip, top, left, out="f32")
    assert f.dtype == torch.float32 and tuple(f.shape) == (len(ragged), 3, S, S) and f.is_contiguous()
    assert torch.equal(f.cpu(), _to_float_host(u8))
    # every byte value through the conversion: a pure crop of a 48 x 48 image holding 0 .. 255
    ramp = (np.arange(48 * 48 * 3) % 256).astype(np.uint8).reshape(48, 48, 3)
    one, _ = _pack([ramp])
    z = torch.zeros(1, dtype=torch.int64)
    u = pipe.apply(one.to(DEV), z, z, z, out="u8")
    assert torch.equal(u[0].cpu(), torch.from_numpy(ramp[:S, :S])) and len(u.unique()) == 256
    fr = pipe.apply(one.to(DEV), z, z, z, out="f32").cpu()
    assert torch.equal(fr, _to_float_host(u))
    assert torch.equal(fr, torch.from_numpy(D.to_float(u.cpu().numpy())))
    xg = u.permute(0, 3, 1, 2).float().div(255)
    print(f"f32 against the same three ops on GPU tensors: {int((fr != xg.add(xg).add_(-1).cpu()).sum())} of {fr.numel()} differ (a * (1 / 255))")


def test_call_draws_then_applies():
    ragged, _ = _pack(SOURCES)
    dev = ragged.to(DEV)
    a = _pipe(generator=torch.Generator().manual_seed(5))
    b = _pipe(generator=torch.Generator().manual_seed(5))
    assert torch.equal(a(dev, out="u8"), b.apply(dev, *b.draw(ragged), out="u8"))


def test_golden_cases_match_pil_bytes():
    """PIL's own flip -> resize -> crop bytes, recorded where PIL is installed (tools/capture_data_golden.py)."""
    g = load_golden("data_pil_lanczos")
    mid, size = int(g["mid"]), int(g["size"])
    pipe = _pipe(size, mid / size)
    assert pipe.mid == mid
    n_src = sum(1 for k in g if k.startswith("src_"))
    srcs, flip, top, left, want = [], [], [], [], []
    for i in range(n_src):
        for (f, t, l), ref in zip(g[f"par_{i}"].tolist(), g[f"out_{i}"]):
            srcs.append(g[f"src_{i}"])
            flip.append(f), top.append(t), left.append(l)
            want.append(torch.from_numpy(ref))
    ragged, _ = _pack(srcs)
    got = pipe.apply(ragged.to(DEV), torch.tensor(flip), torch.tensor(top), torch.tensor(left), out="u8").cpu()
    for j in range(len(srcs)):
        assert torch.equal(got[j], want[j]), (j, srcs[j].shape, flip[j], top[j], left[j])


def test_full_size_against_spec():
    """image_size 256 (mid 384): one 256-thread column block, 16 bands; (375, 500) down-scales slightly, (500, 333) up-scales."""
    rng = np.random.default_rng(3)
    srcs = [rng.integers(0, 256, (375, 500, 3), dtype=np.uint8), rng.integers(0, 256, (500, 333, 3), dtype=np.uint8)]
    srcs[1][::4] = 255
    srcs[1][1::4] = 0
    pipe = _pipe(256)
    ragged, _ = _pack(srcs)
    flip, top, left = torch.tensor([1, 0]), torch.tensor([128, 17]), torch.tensor([255, 128])
    got = pipe.apply(ragged.to(DEV), flip, top, left, out="u8").cpu()
    for i in range(2):
        want = _spec(i, int(flip[i]), int(top[i]), int(left[i]), sources=srcs, mid=384, size=256, tag="full")
        assert torch.equal(got[i], want), f"image {i}: {int((got[i] != want).sum())} bytes differ"


def test_more_than_one_column_block_and_a_ragged_last_band():
    """image_size 264 = 256 + 8 columns (a second column block with 8 live threads) and 16 bands + 8 rows, with mid_reso 1.0 (the crop is as wide as the
    resized shorter edge): sizes the 32- and 256-pixel cases never reach."""
    rng = np.random.default_rng(4)
    srcs = [rng.integers(0, 256, (300, 281, 3), dtype=np.uint8), rng.integers(0, 256, (270, 540, 3), dtype=np.uint8)]
    pipe = _pipe(264, 1.0)
    ragged, _ = _pack(srcs)
    assert pipe.sizes(ragged) == [(281, 264), (264, 528)]
    flip, top, left = torch.tensor([0, 1]), torch.tensor([17, 0]), torch.tensor([0, 264])
    got = pipe.apply(ragged.to(DEV), flip, top, left, out="u8").cpu()
    for i in range(2):
        want = _spec(i, int(flip[i]), int(top[i]), int(left[i]), sources=srcs, mid=264, size=264, tag="wide")
        assert torch.equal(got[i], want), f"image {i}: {int((got[i] != want).sum())} bytes differ"


def test_val_pipeline_feeds_the_encoder():
    """DeviceInputPipeline(mode="val") on the golden sources, then VAE.encode: equal to VAE.encode of the same batch built on the host from the spec, under
    torch.equal -- the inputs are identical bits."""
    from dmvae_amd.data import pack_images
    from dmvae_amd.models.vae import VAE
    g = load_golden("data_pil_lanczos")
    srcs = [g[f"src_{i}"] for i in range(sum(1 for k in g if k.startswith("src_")))]
    pipe = _pipe(256, 1.5, mode="val")
    ragged = pack_images(srcs)
    assert ragged.data.is_pinned()
    x = pipe(ragged.to(DEV, non_blocking=True))
    flip, top, left = pipe.draw(ragged)
    assert not flip.any()
    host = np.stack([D.pipeline(a, 384, 256, 0, int(t), int(l)) for a, t, l in zip(srcs, top, left)])
    xh = torch.from_numpy(D.to_float(host)).to(DEV)
    assert torch.equal(x, xh)
    torch.manual_seed(5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "pretrained weights are not available offline"
        vae = VAE(z_channels=32, model_size="base", encoder_kwargs=dict(embed_dim=256, depth=1, num_heads=4)).to(DEV).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        z, zh = vae.encode(x), vae.encode(xh)
    assert torch.isfinite(z.float()).all() and torch.equal(z, zh)


class _SourceDataset(torch.utils.data.Dataset):
    """The decoded sources as a decode-only DatasetFolder yields them."""

    def __len__(self):
        return len(SOURCES)

    def __getitem__(self, i):
        return SOURCES[i], i


def test_pack_from_dataloader_workers_arrives_pinned():
    """The documented wiring: collate_ragged in two worker processes, pin_memory=True.  The workers neither pin nor open the GPU (tests/test_data_cpu.py);
    the loader's pin thread pins the pack through RaggedImages.pin_memory, so the copy to the device can be asynchronous, and the result is the spec's."""
    from dmvae_amd.data import collate_ragged
    pipe = _pipe(mode="val")
    loader = torch.utils.data.DataLoader(_SourceDataset(), batch_size=4, num_workers=2, pin_memory=True, collate_fn=collate_ragged)
    seen = 0
    for ragged, labels in loader:
        assert ragged.is_pinned() and not ragged.data.is_cuda
        flip, top, left = pipe.draw(ragged)
        got = pipe.apply(ragged.to(DEV, non_blocking=True), flip, top, left, out="u8").cpu()
        for j, i in enumerate(labels.tolist()):
            assert torch.equal(got[j], _spec(i, 0, int(top[j]), int(left[j]))), i
        seen += len(ragged)
    assert seen == len(SOURCES)


def test_image_preprocess_argument_checks():
    from dmvae_amd import _lib, ops
    pipe = _pipe()
    ragged, _ = _pack(SOURCES[:2])
    z = torch.zeros(2, dtype=torch.int64)
    rec, taps = pipe.tables(ragged, z, z, z)
    pack, rec_d, taps_d = ragged.data.to(DEV), rec.to(DEV), taps.to(DEV)
    ok = ops.image_preprocess(pack, rec_d, taps_d, S, "u8")
    assert tuple(ok.shape) == (2, S, S, 3)
    with pytest.raises(_lib.DmvaeHipError):
        ops.image_preprocess(ragged.data, rec_d, taps_d, S, "u8")                       # a host pack
    with pytest.raises(ValueError):
        ops.image_preprocess(pack, rec_d, taps_d, S, "bf16")                            # an unknown output kind
    with pytest.raises(_lib.DmvaeHipError):
        ops.image_preprocess(pack, rec, taps_d, S, "u8")                                # the table left on the host
    with pytest.raises(TypeError):
        ops.image_preprocess(pack, rec_d.int(), taps_d, S, "u8")
    with pytest.raises(TypeError):
        ops.image_preprocess(pack, rec_d, taps_d.long(), S, "u8")
    with pytest.raises(ValueError):
        ops.image_preprocess(pack, rec_d[:, :11].contiguous(), taps_d, S, "u8")         # a record of the wrong width
    with pytest.raises(ValueError):
        ops.image_preprocess(pack, rec_d, taps_d, 0, "u8")
    with pytest.raises(ValueError):
        ops.image_preprocess(pack, rec_d, taps_d, S, "u8", into=torch.empty(2, S, S + 1, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.image_preprocess(pack, rec_d, taps_d, S, "f32", into=torch.empty(2, 3, S, S, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.image_preprocess(pack, rec_d, taps_d, S, "u8", into=torch.empty(2, S, S, 6, dtype=torch.uint8, device=DEV)[..., ::2])   # not contiguous
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            ops.image_preprocess(pack, rec_d.to("cuda:1"), taps_d, S, "u8")
    assert torch.equal(ops.image_preprocess(pack, rec_d, taps_d, S, "u8"), ok)
