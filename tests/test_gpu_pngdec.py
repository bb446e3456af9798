"""mopa_amd/pngdec.py on the device (csrc/pngdec.hip) against Pillow's decoded arrays, read from the fixture
tests/golden/g18_pngdec.npz (written by tests/golden_gen/g18_pngdec.py, which ran Pillow 12.2 and held the restatement
tests/_png_reference.py against it), and against the restatement's rule on hand-made scanlines: PNG is lossless, so the expected
output of any encoded image is ``expand_rgb(original)``.  Nothing here imports Pillow except the fallback test; every comparison is
an equality.

The shapes are the smallest that cross every edge of the kernel's tiling, which the library is asked for: R rows per pass (a wave
takes 64 of them), K columns per block."""
import os
import zlib

import numpy as np
import pytest
import torch

import _png_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_pngdec.npz"))


@pytest.fixture(scope="module")
def pd():
    from mopa_amd import pngdec
    return pngdec


@pytest.fixture(scope="module")
def tiling(pd):
    from mopa_amd import _lib
    return _lib.query("mopa_png_rows_per_pass"), _lib.query("mopa_png_block_cols"), _lib.query("mopa_png_max_images")


PALETTE = np.random.Generator(np.random.PCG64(7)).integers(0, 256, (256, 3), dtype=np.uint8)


def case(pd, img, ct, filters):
    """(header, host buffer of hand-made scanlines, expected RGB)"""
    px = ref.as_pixels(img, ct)
    rows = ref.filter_rows(px, ct, filters)
    return (ref.header_for(pd, px.shape[1], px.shape[0], ct, PALETTE if ct == 3 else None), torch.from_numpy(rows.reshape(-1).copy()),
            ref.expand_rgb(px, ct, PALETTE))


def run_cases(pd, cases, what):
    got = pd.decode_scanlines_batch([c[0] for c in cases], [c[1] for c in cases])
    for k, (c, t) in enumerate(zip(cases, got)):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == c[2].shape, (what, k)
        host = t.cpu().numpy()
        assert np.array_equal(host, c[2]), (what, k, c[2].shape, int((host != c[2]).sum()))
    return got


def test_fixture_streams_equal_pillow(pd, fx):
    names = [str(n) for n in fx["names"]]
    got = pd.decode_png_batch([fx[f"{n}_png"].tobytes() for n in names])
    for n, t in zip(names, got):
        assert torch.equal(t.cpu(), torch.from_numpy(fx[f"{n}_rgb"])), n
    alone = pd.decode_png_batch([fx["pal_short_png"].tobytes()], threads=1)[0]
    assert torch.equal(alone, got[names.index("pal_short")])


@pytest.mark.parametrize("ct", ref.COLOR_TYPES)
def test_smallest_images_first_row_first_pixel_and_each_filter(pd, ct):
    """1 x 1, 1 x W, H x 1; every filter on the first row (the row above is zeros) and on the first pixel; images whose rows all use
    one filter, for each filter; a mixed cycle."""
    rng = np.random.Generator(np.random.PCG64(100 + ct))
    cases = []
    for f in range(5):
        cases.append(case(pd, ref.random_image(rng, 1, 1, ct), ct, f))
        cases.append(case(pd, ref.random_image(rng, 1, 9, ct), ct, f))
        cases.append(case(pd, ref.random_image(rng, 9, 1, ct), ct, f))
        cases.append(case(pd, ref.random_image(rng, 11, 13, ct), ct, f))
        cases.append(case(pd, ref.random_image(rng, 6, 7, ct), ct, [f] + [(f + k) % 5 for k in range(1, 6)]))
    cases.append(case(pd, ref.random_image(rng, 23, 17, ct), ct, np.arange(23) % 5))
    cases.append(case(pd, ref.random_image(rng, 23, 17, ct), ct, (np.arange(23) * 3 + 4) % 5))
    run_cases(pd, cases, f"colour type {ct}")


def test_paeth_ties(pd):
    """An all-equal image (pa == pb == pc == 0 inside, pa == pb on the first row and column) and two-valued images: every tie of
    the Paeth choice, which prefers a, then b."""
    rng = np.random.Generator(np.random.PCG64(5))
    cases = []
    for ct in ref.COLOR_TYPES:
        cases.append(case(pd, np.full((9, 11, ref.BPP[ct]), 37, np.uint8), ct, 4))
        two = np.where(rng.random((17, 19, ref.BPP[ct])) < 0.5, 10, 200).astype(np.uint8)
        cases.append(case(pd, two, ct, 4))
        cases.append(case(pd, two, ct, np.arange(17) % 5))
    # the ties named in the issue, by construction: a row above of (c, b) = (10, 200), a = 200: pa == pb; and b == c: pb == pc > pa ...
    tie = np.asarray([[10, 200, 200, 10], [200, 200, 10, 10], [10, 10, 10, 200]], np.uint8)
    cases.append(case(pd, tie, 0, 4))
    run_cases(pd, cases, "ties")


def test_every_tile_edge(pd, tiling):
    R, K, _ = tiling
    rng = np.random.Generator(np.random.PCG64(6))
    shapes = [(H, 5) for H in (63, 64, 65, R - 1, R, R + 1, 2 * R + 1)] + [(70, W) for W in (K - 1, K, K + 1, 2 * K + 1)]
    for ct in ref.COLOR_TYPES:
        cases = [case(pd, rng.integers(0, 256, (H, W, ref.BPP[ct]), dtype=np.uint8), ct, rng.integers(0, 5, H)) for H, W in shapes]
        run_cases(pd, cases, f"tile edges, colour type {ct}")


def test_one_call_over_the_chunk_boundary_and_destinations(pd, tiling, fx):
    """Mixed sizes and colour types and max_images + 1 tiny images: two launches, one copy each; then out= views with a wider
    pitch, the refusals of out=, and two consecutive calls with other content (the staging buffer's fence)."""
    _, _, M = tiling
    rng = np.random.Generator(np.random.PCG64(8))
    imgs, datas = [], []
    for k in range(M + 1):
        ct = ref.COLOR_TYPES[k % 5]
        img = ref.random_image(rng, 1 + k % 7, 1 + (k * 5) % 11, ct)
        imgs.append(ref.expand_rgb(img, ct, PALETTE))
        datas.append(ref.encode_png(img, ct, rng.integers(0, 5, img.shape[0]), palette=PALETTE if ct == 3 else None))
    calls = []
    orig = pd.call
    pd.call = lambda nm, *a: (calls.append((nm, a[4])), orig(nm, *a))[1]
    try:
        got = pd.decode_png_batch(datas)
    finally:
        pd.call = orig
    assert calls == [("mopa_png_decode_batch", M), ("mopa_png_decode_batch", 1)]
    for k, (t, want) in enumerate(zip(got, imgs)):
        assert np.array_equal(t.cpu().numpy(), want), k
    # a second call with other content right behind the first
    again = pd.decode_png_batch(list(reversed(datas)), threads=1)
    for k, (t, want) in enumerate(zip(again, reversed(imgs))):
        assert np.array_equal(t.cpu().numpy(), want), k
    # destinations: a window of a wider buffer, at every byte alignment
    data, want = fx["ct2_mixed_png"].tobytes(), torch.from_numpy(fx["ct2_mixed_rgb"]).cuda()
    H, W, _ = want.shape
    for pad_px, x_px in ((5, 0), (7, 3), (4, 1)):
        big = torch.full((H + 2, W + pad_px + x_px, 3), 201, dtype=torch.uint8, device="cuda")
        view = big[1:H + 1, x_px:x_px + W]
        res = pd.decode_png_batch([data], out=[view])
        assert res[0] is view and torch.equal(view, want), (pad_px, x_px)
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[1:H + 1, x_px:x_px + W] = False
        assert (big[mask] == 201).all(), (pad_px, x_px)
    buf = torch.zeros(H + 4, W, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=r"out\[1\] overlaps out\[0\]"):
        pd.decode_png_batch([data, data], out=[buf[:H], buf[4:]])
    with pytest.raises(ValueError, match=rf"must be \({H}, {W}, 3\)"):
        pd.decode_png_batch([data], out=[buf])
    with pytest.raises(TypeError, match="uint8"):
        pd.decode_png_batch([data], out=[torch.zeros(H, W, 3, device="cuda")])
    with pytest.raises(ValueError, match="strides"):
        pd.decode_png_batch([data], out=[torch.zeros(H, 3, W, dtype=torch.uint8, device="cuda").permute(0, 2, 1)])
    with pytest.raises(TypeError, match="host bytes"):
        pd.decode_png_batch([torch.from_numpy(fx["ct2_mixed_png"]).cuda()])
    assert not buf.any()


def test_refused_and_malformed_streams_raise_before_any_launch(pd, fx):
    good = fx["ct2_mixed_png"].tobytes()
    calls = []
    orig = pd.call
    pd.call = lambda nm, *a: (calls.append(nm), orig(nm, *a))[1]
    try:
        for n in list(fx["refused"]) + list(fx["malformed"]):
            exc = pd.PngUnsupported if str(n).startswith("refused") else pd.PngDataError
            with pytest.raises(exc, match=r"datas\[1\]"):
                pd.decode_png_batch([good, fx[f"{n}_png"].tobytes()])
        assert calls == []
        after = pd.decode_png_batch([good])[0]
    finally:
        pd.call = orig
    assert calls == ["mopa_png_decode_batch"] and torch.equal(after.cpu(), torch.from_numpy(fx["ct2_mixed_rgb"]))
    # the entry point checks again what the kernel's indexing rests on
    hdr, buf = pd.inflate_scanlines(good)
    with pytest.raises(ValueError, match="the header's scanlines"):
        pd.decode_scanlines_batch([hdr], [buf[:-1]])
    hdr.bpp = 4
    with pytest.raises(ValueError, match="not a supported image"):
        pd.decode_scanlines_batch([hdr], [buf])
    out = [torch.empty(32, 32, 3, dtype=torch.uint8, device="cuda")]
    with pytest.raises(RuntimeError, match="mopa_png_decode_batch failed with code -1"):
        pd._launch([hdr], out[0].data_ptr(), [buf.cuda()], [buf.numel()], out)


@pytest.fixture(scope="module")
def full_size(pd):
    """The two camera shapes, seeded synthetic RGB, all five filters cycling: (source array, decoded tensor) each."""
    res = []
    for k, (H, W) in enumerate(((376, 1241), (1208, 1920))):
        img = ref.synthetic_rgb(H, W, 18 + k)
        res.append((img, pd.decode_png_batch([ref.encode_png(img, 2, np.arange(H) % 5, level=1)])[0]))
    return res


def test_full_size_checksums(full_size):
    for img, t in full_size:
        assert tuple(t.shape) == img.shape
        assert zlib.crc32(t.cpu().numpy().tobytes()) == zlib.crc32(img.tobytes()), img.shape


def test_chain_into_resize(full_size):
    from mopa_amd import imageprep as ip
    img, t = full_size[0]
    assert torch.equal(ip.resize_bilinear_u8([t], (400, 120)), ip.resize_bilinear_u8([torch.from_numpy(img).cuda()], (400, 120)))


def test_decode_images_mixed_list_and_fallback(pd, fx, golden_dir):
    from mopa_amd import imagedec, jpegdec
    g16 = np.load(os.path.join(golden_dir, "g16_jpegdec.npz"))
    jpg = g16["s420_40x56_jpg"].tobytes()
    pngs = [fx["ct6_mixed_png"].tobytes(), fx["pil_P_png"].tobytes()]
    got = imagedec.decode_images([pngs[0], jpg, pngs[1]])
    sep_j, sep_p = jpegdec.decode_jpeg_batch([jpg]), pd.decode_png_batch(pngs)
    assert torch.equal(got[0], sep_p[0]) and torch.equal(got[1], sep_j[0]) and torch.equal(got[2], sep_p[1])
    assert torch.equal(got[1].cpu(), torch.from_numpy(g16["s420_40x56_rgb"]))
    laced = fx["refused_adam7_png"].tobytes()
    with pytest.raises(pd.PngUnsupported, match="Adam7"):
        imagedec.decode_images([pngs[0], laced], fallback=False)
    with pytest.raises(pd.PngDataError):
        imagedec.decode_images([pngs[0], fx["bad_crc_png"].tobytes()])
    with pytest.raises(ValueError, match="neither a JPEG nor a PNG"):
        imagedec.decode_images([b"GIF89a..."])
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(pd.PngUnsupported, match="Adam7"):
            imagedec.decode_images([pngs[0], laced])
    else:
        both = imagedec.decode_images([laced, pngs[0]])
        assert both[0].is_cuda and torch.equal(both[0].cpu(), torch.from_numpy(fx["refused_adam7_rgb"])) and torch.equal(both[1], sep_p[0])
