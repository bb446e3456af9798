"""The host side of mopa_amd/pngdec.py without a GPU: the numpy restatement tests/_png_reference.py against the fixture
tests/golden/g18_pngdec.npz (always: Pillow's decoded arrays, written by tests/golden_gen/g18_pngdec.py) and against Pillow (where it
can be imported), ``png_info``, ``inflate_scanlines`` against the restatement's filtered bytes, every refusal with its reason, and the
cap on what a hostile stream can make inflate produce."""
import io
import os
import zlib

import numpy as np
import pytest
import torch

import _png_reference as ref
from mopa_amd import pngdec as pd


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_pngdec.npz"))


@pytest.fixture(scope="module")
def names(fx):
    return [str(n) for n in fx["names"]]


def stream(fx, name):
    return fx[f"{name}_png"].tobytes()


def test_fixture_covers_the_supported_set(fx, names):
    seen = set()
    for n in names:
        _, _, ct, _, rows = ref.scanlines(stream(fx, n))
        seen |= {(ct, int(f)) for f in rows[:, 0]}
    assert seen == {(ct, f) for ct in ref.COLOR_TYPES for f in range(5)}
    assert {"pal_short", "pal_trns", "rgb_trns", "idat3", "idat_empty", "ancillary"} <= set(names)
    kinds = [k for k, _ in ref.chunks(stream(fx, "idat_empty"))]
    assert kinds.count(b"IDAT") == 4 and any(k == b"IDAT" and len(b) == 0 for k, b in ref.chunks(stream(fx, "idat_empty")))
    assert [k for k, _ in ref.chunks(stream(fx, "ancillary"))][:4] == [b"IHDR", b"gAMA", b"tEXt", b"prVt"]
    _, _, _, _, rows = ref.scanlines(stream(fx, "pal_short"))
    assert len(dict(ref.chunks(stream(fx, "pal_short")))[b"PLTE"]) == 21 and rows[:, 1:].max() >= 7


def test_restatement_equals_pillows_arrays(fx, names):
    """The rule: PNG is lossless, the output is expand_rgb of what was encoded -- which is what Pillow's convert("RGB") gave."""
    for n in names:
        px, ct, pal = ref.decode_png(stream(fx, n))
        assert np.array_equal(ref.expand_rgb(px, ct, pal), fx[f"{n}_rgb"]), n


def test_encoder_round_trip_and_vectorised_filtering():
    rng = np.random.Generator(np.random.PCG64(3))
    pal = rng.integers(0, 256, (200, 3), dtype=np.uint8)
    for ct in ref.COLOR_TYPES:
        img = ref.random_image(rng, 7, 11, ct)
        data = ref.encode_png(img, ct, rng.integers(0, 5, 7), palette=pal if ct == 3 else None, idat_split=2)
        px, ct2, _ = ref.decode_png(data)
        assert ct2 == ct and np.array_equal(px, img)


def test_restatement_equals_pillow_where_importable(fx, names):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.Generator(np.random.PCG64(4))
    datas = [stream(fx, n) for n in names]
    datas += [ref.encode_png(ref.random_image(rng, 12, 17, ct), ct, rng.integers(0, 5, 12), palette=rng.integers(0, 256, (256, 3), dtype=np.uint8)
                             if ct == 3 else None) for ct in ref.COLOR_TYPES]
    for data in datas:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        px, ct, pal = ref.decode_png(data)
        assert np.array_equal(ref.expand_rgb(px, ct, pal), want)


def test_png_info(fx):
    assert pd.png_info(stream(fx, "pil_RGB")) == pd.PngInfo((19, 21), "RGB", 8, False, True, None)
    for mode in ("L", "P", "LA", "RGBA"):
        i = pd.png_info(stream(fx, f"pil_{mode}"))
        assert (i.size, i.mode, i.bit_depth, i.interlaced, i.supported, i.reason) == ((19, 21), mode, 8, False, True, None)
    i = pd.png_info(memoryview(stream(fx, "refused_16bit")))
    assert (i.size, i.mode, i.bit_depth, i.supported) == ((13, 9), None, 16, False) and "16-bit" in i.reason
    i = pd.png_info(np.frombuffer(stream(fx, "refused_4bit"), np.uint8))
    assert (i.bit_depth, i.supported) == (4, False) and "4-bit" in i.reason
    i = pd.png_info(torch.from_numpy(fx["refused_adam7_png"]))
    assert i.interlaced and not i.supported and "Adam7" in i.reason and i.mode == "RGB"
    big = ref.wrap(8193, 1, 0, zlib.compress(b"\0" * 8194))
    assert pd.png_info(big).supported is False and "8192" in pd.png_info(big).reason
    apng = ref.encode_png(np.zeros((2, 2), np.uint8), 0, 0, extra_chunks=[(b"acTL", b"\0\0\0\1\0\0\0\0")])
    assert not pd.png_info(apng).supported and "APNG" in pd.png_info(apng).reason
    with pytest.raises(pd.PngDataError, match="signature"):
        pd.png_info(b"\xff\xd8\xff\xe0 not a png")
    with pytest.raises(TypeError):
        pd.png_info("a path")


def test_inflate_scanlines_returns_the_filtered_bytes(fx, names):
    for n in names:
        data = stream(fx, n)
        W, H, ct, pal, rows = ref.scanlines(data)
        hdr, buf = pd.inflate_scanlines(data)
        assert (hdr.width, hdr.height, hdr.color_type, hdr.bpp) == (W, H, ct, ref.BPP[ct]), n
        assert hdr.stride == W * ref.BPP[ct] and hdr.scan_bytes == rows.size == buf.numel()
        assert buf.dtype == torch.uint8 and np.array_equal(buf.numpy(), rows.reshape(-1)), n
        table = np.ctypeslib.as_array(hdr.palette)
        if ct == 3:
            assert np.array_equal(table, pal[:, 0].astype(np.uint32) | pal[:, 1].astype(np.uint32) << 8 | pal[:, 2].astype(np.uint32) << 16), n
        else:
            assert not table.any()
    # the palette is zero past PLTE
    hdr, _ = pd.inflate_scanlines(stream(fx, "pal_short"))
    assert np.ctypeslib.as_array(hdr.palette)[:7].any() and not np.ctypeslib.as_array(hdr.palette)[7:].any()
    # out=: filled in place, too short is refused
    data = stream(fx, "ct2_mixed")
    rows = ref.scanlines(data)[4]
    out = np.full(rows.size + 5, 7, np.uint8)
    hdr, buf = pd.inflate_scanlines(data, out=out)
    assert np.array_equal(out[:rows.size], rows.reshape(-1)) and (out[rows.size:] == 7).all() and buf.numel() == rows.size
    with pytest.raises(ValueError, match="out holds"):
        pd.inflate_scanlines(data, out=np.zeros(rows.size - 1, np.uint8))


def test_refusals(fx):
    for n, why in (("refused_16bit", "16-bit samples"), ("refused_4bit", "4-bit samples"), ("refused_adam7", "Adam7 interlace")):
        with pytest.raises(pd.PngUnsupported, match=why):
            pd.inflate_scanlines(stream(fx, n))
    apng = ref.encode_png(np.zeros((2, 2), np.uint8), 0, 0, extra_chunks=[(b"acTL", b"\0\0\0\1\0\0\0\0")])
    with pytest.raises(pd.PngUnsupported, match="APNG"):
        pd.inflate_scanlines(apng)
    for n, why in (("bad_crc", "CRC"), ("bad_truncated", "inflate to 178 bytes, the header promises 360"), ("bad_filter5", "filter byte 5"),
                   ("bad_trailing", "inflate to more bytes")):
        with pytest.raises(pd.PngDataError, match=why):
            pd.inflate_scanlines(stream(fx, n))
    assert [str(n) for n in fx["malformed"]] == ["bad_crc", "bad_truncated", "bad_filter5", "bad_trailing"]
    good = stream(fx, "ct2_mixed")
    rows = ref.filter_rows(np.zeros((3, 4, 3), np.uint8), 2, 0).tobytes()
    comp = zlib.compress(rows)
    cases = {
        "signature": b"\x89PNG\r\n\x1a\r" + good[8:],
        "empty": b"",
        "no IEND": good[:-12],
        "cut inside a chunk": good[:len(good) // 2],
        "the first chunk is not IHDR": ref.SIGNATURE + ref.chunk(b"IDAT", comp) + ref.chunk(b"IEND"),
        "no IDAT": ref.SIGNATURE + ref.ihdr(4, 3, 2) + ref.chunk(b"IEND"),
        "no PLTE": ref.wrap(4, 3, 3, zlib.compress(ref.filter_rows(np.zeros((3, 4), np.uint8), 3, 0).tobytes())),
        "zero side": ref.wrap(0, 3, 2, comp),
        "inflate error": ref.wrap(4, 3, 2, b"\x78\x9c" + b"\xff" * 20),
        "no end of the compressed stream": ref.wrap(4, 3, 2, zlib.compressobj().compress(rows) + zlib.compressobj(wbits=-15).flush()),
        "colour type": ref.wrap(4, 3, 5, comp),
        "unknown critical chunk": ref.encode_png(np.zeros((3, 4, 3), np.uint8), 2, 0, extra_chunks=[(b"ABCD", b"")]),
    }
    for what, data in cases.items():
        with pytest.raises(pd.PngDataError):
            pd.inflate_scanlines(data)
        pytest.raises(pd.PngDataError, pd.png_info, data) if what not in ("inflate error", "no end of the compressed stream") else None
    assert issubclass(pd.PngUnsupported, ValueError) and issubclass(pd.PngDataError, ValueError)


def test_inflate_is_capped_one_byte_past_the_header(monkeypatch):
    """A stream whose image data inflate to 64 MiB behind a 4 x 3 header: refused, and inflate was never asked for more than
    need + 1 bytes nor produced more."""
    need = 3 * (1 + 4 * 3)
    bomb = ref.wrap(4, 3, 2, zlib.compress(b"\0" * (64 << 20), 9))
    assert len(bomb) < 1 << 17
    asked, made = [], []
    real = zlib.decompressobj

    class Spy:
        def __init__(self):
            self.d = real()

        def decompress(self, data, max_length=0):
            asked.append(max_length)
            out = self.d.decompress(data, max_length)
            made.append(len(out))
            return out

        eof = property(lambda self: self.d.eof)

    monkeypatch.setattr(pd.zlib, "decompressobj", Spy)
    with pytest.raises(pd.PngDataError, match="inflate to more bytes"):
        pd.inflate_scanlines(bomb)
    assert asked == [need + 1] and made == [need + 1]
