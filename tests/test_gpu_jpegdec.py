"""mopa_amd/jpegdec.py on the device (csrc/jpegdec.hip behind csrc/jpeg_entropy.h) against Pillow's decoded arrays, read from the
fixture tests/golden/g16_jpegdec.npz (written by tests/golden_gen/g16_jpegdec.py, which ran Pillow 12.2 / libjpeg-turbo and held
the restatement tests/_jpeg_reference.py against it).  Nothing here imports Pillow; every comparison is an equality.

The small cases (tests/_jpeg_reference.py::small_cases, 64 of them) are the smallest shapes at which each part can go wrong: widths
1, 7, 8, 9, 15, 16, 17, 33 and heights 1, 8, 9, 16, 17 with each of 4:4:4 / 4:2:2 / 4:2:0 (single-sample chroma planes and planes of
two columns, which the library replicates; partial MCUs on either side; the upsampler's first and last column and row; full
four-pixel groups and 1-, 2- and 3-pixel tails; rows at every byte alignment), qualities 10 / 75 / 100, optimised Huffman tables,
restart intervals 1 and 3, a grey image, a 40 x 56 image per sampling.  Full size: 1600 x 900 4:2:0 by CRC32 and byte sum."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "g16_jpegdec.npz"))


@pytest.fixture(scope="module")
def names(fx):
    return [str(n) for n in fx["names"]]


@pytest.fixture(scope="module")
def jd():
    from mopa_amd import jpegdec
    return jpegdec


def stream(fx, name):
    return fx[f"{name}_jpg"].tobytes()


def want(fx, name):
    return torch.from_numpy(fx[f"{name}_rgb"])


@pytest.fixture(scope="module")
def alone(jd, fx, names):
    """1. every small case decoded alone (computed once; the other tests compare with it)."""
    return {n: jd.decode_jpeg_batch([stream(fx, n)])[0] for n in names}


def test_every_small_case_alone_equals_pillow(fx, names, alone):
    for n in names:
        t = alone[n]
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == tuple(fx[f"{n}_rgb"].shape), n
        got = t.cpu()
        assert torch.equal(got, want(fx, n)), (n, int((got != want(fx, n)).sum()))


def test_all_small_cases_in_one_call(jd, fx, names, alone):
    """2. more than 32 images of mixed sizes and samplings: the chunk walk and the pointer tables; one upload and one launch per
    chunk; the pool and the calling thread give the same bytes."""
    assert len(names) > 2 * 32 - 1
    calls = []
    orig = jd.call
    jd.call = lambda nm, *a: (calls.append((nm, a[3])), orig(nm, *a))[1]
    try:
        together = jd.decode_jpeg_batch([stream(fx, n) for n in names])
    finally:
        jd.call = orig
    assert calls == [("mopa_jpeg_decode_batch", 32), ("mopa_jpeg_decode_batch", len(names) - 32)]
    for n, t in zip(names, together):
        assert torch.equal(t, alone[n]), n
    single = jd.decode_jpeg_batch([stream(fx, n) for n in reversed(names)], threads=1)
    for n, t in zip(reversed(names), single):
        assert torch.equal(t, alone[n]), n


def test_destination_variants(jd, fx, alone):
    """3. a row pitch wider than 3 W, and an odd width that leaves rows unaligned: the image equals the plain call, the bytes
    outside it are untouched."""
    for n in ("s420_40x56", "s422_33x9", "s444_15x17", "s420_7x8", "grey_33x17", "s420_1x1"):
        data, ref = stream(fx, n), alone[n]
        H, W, _ = ref.shape
        for pad_px, x_px in ((5, 0), (7, 3), (4, 1)):           # wider pitch; windows that start at every byte alignment
            big = torch.full((H + 2, W + pad_px + x_px, 3), 201, dtype=torch.uint8, device="cuda")
            view = big[1:H + 1, x_px:x_px + W]
            res = jd.decode_jpeg_batch([data], out=[view])
            assert res[0] is view and torch.equal(view, ref), (n, pad_px, x_px)
            mask = torch.ones_like(big, dtype=torch.bool)
            mask[1:H + 1, x_px:x_px + W] = False
            assert (big[mask] == 201).all(), (n, pad_px, x_px)
        # a contiguous destination of an odd width: every row starts at another alignment
        flat = torch.full((H * W * 3 + 8,), 77, dtype=torch.uint8, device="cuda")
        for shift in (0, 1, 2, 3):
            flat.fill_(77)
            view = flat[shift:shift + H * W * 3].view(H, W, 3)
            jd.decode_jpeg_batch([data], out=[view])
            assert torch.equal(view, ref) and (flat[:shift] == 77).all() and (flat[shift + H * W * 3:] == 77).all(), (n, shift)


def test_out_is_checked(jd, fx, alone):
    data, ref = stream(fx, "s420_40x56"), alone["s420_40x56"]
    buf = torch.zeros(60, 40, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match=r"out\[1\] overlaps out\[0\]"):
        jd.decode_jpeg_batch([data, data], out=[buf[:56], buf[4:]])
    with pytest.raises(ValueError, match=r"must be \(56, 40, 3\)"):
        jd.decode_jpeg_batch([data], out=[buf])
    with pytest.raises(TypeError, match="uint8"):
        jd.decode_jpeg_batch([data], out=[torch.zeros(56, 40, 3, device="cuda")])
    with pytest.raises(ValueError, match="strides"):
        jd.decode_jpeg_batch([data], out=[torch.zeros(56, 3, 40, dtype=torch.uint8, device="cuda").permute(0, 2, 1)])
    with pytest.raises(TypeError, match="host bytes"):
        jd.decode_jpeg_batch([torch.from_numpy(fx["s420_40x56_jpg"]).cuda()])
    assert not buf.any()
    out = [torch.empty_like(ref), torch.empty_like(ref)]
    assert jd.decode_jpeg_batch([data, data], out=out) == out and torch.equal(out[0], ref) and torch.equal(out[1], ref)


def test_device_stage_alone_on_the_fixture_coefficients(jd, fx, names):
    """4. the device half fed with the fixture's coefficient planes (the restatement's), bypassing the library's entropy stage."""
    hdrs, bufs = [], []
    for n in names:
        g = fx[f"{n}_geom"]
        planes = [fx[f"{n}_c{c}"] for c in range(int(g[2]))]
        h, b = jd.pack_coefficients((int(g[0]), int(g[1])), planes, fx[f"{n}_quant"], (int(g[3]), int(g[4])))
        hdrs.append(h)
        bufs.append(b)
    got = jd.decode_coefficients_batch(hdrs, bufs)
    for n, t in zip(names, got):
        assert torch.equal(t.cpu(), want(fx, n)), n
    # device-resident coefficient buffers are taken as they are
    k = names.index("s420_40x56")
    again = jd.decode_coefficients_batch([hdrs[k]], [bufs[k].cuda()])
    assert torch.equal(again[0], got[k])


def test_full_size_checksums(jd, fx, golden_dir):
    """5. 1600 x 900, 4:2:0: Pillow's CRC32 and byte sum; twice in one call (the second image's tables and offsets)."""
    full = json.load(open(os.path.join(golden_dir, "g16_jpegdec_fullsize.json")))
    data = stream(fx, "full")
    a, b = jd.decode_jpeg_batch([data, data])
    assert tuple(a.shape) == (full["size"][1], full["size"][0], 3)
    host = a.cpu().numpy()
    assert int(host.sum(dtype=np.uint64)) == full["sum"] and zlib.crc32(host.tobytes()) == full["crc32"]
    assert torch.equal(a, b)


def test_chain_into_prepare_batch(jd, fx):
    """6. decode_jpeg_batch -> imageprep.prepare_batch (resize, jitter, flip, normalisation) equals, bit for bit, prepare_batch on
    Pillow's decoded arrays; resize_bilinear_u8 takes the result as it is."""
    from mopa_amd import imageprep as ip
    ns = ["s444_40x56", "s422_40x56", "s420_40x56"]
    dec = jd.decode_jpeg_batch([stream(fx, n) for n in ns])
    pil = [want(fx, n).cuda() for n in ns]
    pts = torch.tensor([[3.0, 4.0], [50.0, 30.0], [20.5, 11.25]], device="cuda")
    jitter = ((0, 1, 2, 3), (1.2, 0.8, 1.1, 0.05))

    def samples(imgs):
        return [{"image": im, "points_img": pts, "flip": b == 1, "jitter": jitter if b != 2 else None} for b, im in enumerate(imgs)]

    got = ip.prepare_batch(samples(dec), resize=(24, 32))
    exp = ip.prepare_batch(samples(pil), resize=(24, 32))
    assert got["img"].shape == (3, 3, 32, 24) and torch.equal(got["img"].view(torch.int32), exp["img"].view(torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(got["img_indices"], exp["img_indices"]))
    assert torch.equal(ip.resize_bilinear_u8(dec, (20, 28)), ip.resize_bilinear_u8(pil, (20, 28)))


def test_refused_and_malformed_streams_raise_before_any_launch(jd, fx, alone):
    """7. nothing is launched for a call with a refused or malformed stream, and a following decode is still correct."""
    good = stream(fx, "s420_40x56")
    calls = []
    orig = jd.call
    jd.call = lambda nm, *a: (calls.append(nm), orig(nm, *a))[1]
    try:
        for bad, exc in ((stream(fx, "refused_progressive"), jd.JpegUnsupported), (stream(fx, "refused_1x2"), jd.JpegUnsupported),
                         (good[:len(good) // 2], jd.JpegDataError), (good[:-2], jd.JpegDataError), (b"", jd.JpegDataError)):
            out = [torch.full((56, 40, 3), 9, dtype=torch.uint8, device="cuda") for _ in range(2)]
            with pytest.raises(exc, match=r"datas\[1\]"):
                jd.decode_jpeg_batch([good, bad], out=out) if exc is jd.JpegDataError else jd.decode_jpeg_batch([good, bad])
            assert calls == [] and all((t == 9).all() for t in out)
        after = jd.decode_jpeg_batch([good])[0]
    finally:
        jd.call = orig
    assert calls == ["mopa_jpeg_decode_batch"] and torch.equal(after, alone["s420_40x56"]) and torch.equal(after.cpu(), want(fx, "s420_40x56"))
