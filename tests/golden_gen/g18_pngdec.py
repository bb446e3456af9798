"""Generate tests/golden/g18_pngdec.npz by RUNNING Pillow: small PNG streams, written by Pillow or encoded by hand
(tests/_png_reference.py::encode_png, the filter of every row forced), and Pillow's decode of each
(``np.asarray(Image.open(...).convert("RGB"))``).

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixture is what travels).
Usage, from the repo root:  python tests/golden_gen/g18_pngdec.py

Refuses to write unless the numpy restatement (``decode_png`` + ``expand_rgb``) equals Pillow on every accepted stream.

Contents of the npz:
  names                 the accepted streams, in order
  <name>_png            the stream, uint8
  <name>_rgb            Pillow's decoded (H, W, 3) uint8 array
  refused               names of well-formed streams outside the supported subset: <name>_png, <name>_rgb (Pillow decodes them)
  malformed             names of malformed streams: <name>_png

Accepted: ``pil_<mode>`` written by Image.save for L / RGB / P / LA / RGBA; ``ct<colour type>_f<filter>`` 13 x 9 with every row
on one filter, for the five colour types x the five filters; ``ct<colour type>_mixed`` 32 x 32 with the filters cycling;
``pal_short`` whose indices exceed the PLTE length; ``pal_trns`` / ``rgb_trns`` / ``grey_trns`` with a tRNS chunk;
``idat3`` (three IDAT chunks), ``idat_empty`` (an empty IDAT chunk among them); ``ancillary`` (gAMA, tEXt and a private chunk
between IHDR and IDAT).  Refused: ``refused_16bit``, ``refused_4bit`` (a 4-bit palette image), ``refused_adam7``.  Malformed:
``bad_crc``, ``bad_truncated`` (the compressed stream is cut), ``bad_filter5``, ``bad_trailing`` (one more row than the header
promises).
"""
import io
import os
import struct
import sys
import warnings
import zlib

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _png_reference as ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g18_pngdec.npz")
MODES = {"L": 0, "RGB": 2, "P": 3, "LA": 4, "RGBA": 6}


def pillow_decode(data):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # "palette images with transparency expressed in bytes should be converted to RGBA"
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def smooth(rng, H, W, bpp):
    """Smooth enough that an adaptive encoder uses several filters."""
    yy, xx = np.mgrid[0:H, 0:W]
    ch = [128 + 90 * np.sin(0.3 * (k + 1) * xx + 0.2 * yy + k) + rng.normal(0, 3, (H, W)) for k in range(bpp)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def main():
    rng = np.random.Generator(np.random.PCG64(18))
    d, names = {}, []
    palette = rng.integers(0, 256, (256, 3), dtype=np.uint8)

    def accept(name, data):
        want = pillow_decode(data)
        px, ct, pal = ref.decode_png(data)
        got = ref.expand_rgb(px, ct, pal)
        if got.shape != want.shape or not np.array_equal(got, want):
            raise SystemExit(f"the restatement differs from Pillow on {name}: nothing written")
        names.append(name)
        d[f"{name}_png"], d[f"{name}_rgb"] = np.frombuffer(data, np.uint8), want

    used = set()
    for mode, ct in MODES.items():
        img = smooth(rng, 21, 19, ref.BPP[ct])
        im = Image.fromarray(img[:, :, 0] if ct in (0, 3) else img, mode if mode != "P" else "L")
        if mode == "P":
            im = Image.fromarray(img[:, :, 0], "P")
            im.putpalette(palette.tobytes())
        buf = io.BytesIO()
        im.save(buf, "PNG")
        data = buf.getvalue()
        assert ref.scanlines(data)[2] == ct, (mode, ref.scanlines(data)[2])
        used |= set(ref.scanlines(data)[4][:, 0].tolist())
        accept(f"pil_{mode}", data)
    print("filters Pillow's encoder chose:", sorted(used))
    for ct in ref.COLOR_TYPES:
        for f in range(5):
            accept(f"ct{ct}_f{f}", ref.encode_png(ref.random_image(rng, 9, 13, ct), ct, f, palette if ct == 3 else None))
        accept(f"ct{ct}_mixed", ref.encode_png(smooth(rng, 32, 32, ref.BPP[ct]), ct, np.arange(32) % 5, palette if ct == 3 else None))
    idx = rng.integers(0, 256, (9, 13), dtype=np.uint8)
    assert (idx >= 7).any()
    accept("pal_short", ref.encode_png(idx, 3, np.arange(9) % 5, palette[:7]))
    accept("pal_trns", ref.encode_png(idx, 3, np.arange(9) % 5, palette, trns=rng.integers(0, 256, 40, dtype=np.uint8).tobytes()))
    rgb = ref.random_image(rng, 9, 13, 2)
    accept("rgb_trns", ref.encode_png(rgb, 2, 4, trns=struct.pack(">HHH", *rgb[3, 4])))
    accept("grey_trns", ref.encode_png(idx, 0, 3, trns=struct.pack(">H", int(idx[2, 2]))))
    accept("idat3", ref.encode_png(rgb, 2, np.arange(9) % 5, idat_split=3))
    z = len(zlib.compress(ref.filter_rows(rgb, 2, np.arange(9) % 5).tobytes(), 6))
    accept("idat_empty", ref.encode_png(rgb, 2, np.arange(9) % 5, idat_split=[0, z // 2, z // 2]))
    accept("ancillary", ref.encode_png(rgb, 2, np.arange(9) % 5, extra_chunks=[(b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"Title\0fixture"),
                                                                              (b"prVt", b"\1\2\3")]))
    d["names"] = np.asarray(names)
    # well-formed streams outside the supported subset
    refused = {}
    buf = io.BytesIO()
    Image.fromarray((rng.integers(0, 65536, (9, 13))).astype(np.uint16)).save(buf, "PNG")
    refused["refused_16bit"] = buf.getvalue()
    im = Image.fromarray(rng.integers(0, 16, (9, 13), dtype=np.uint8), "P")
    im.putpalette(palette[:16].tobytes())
    buf = io.BytesIO()
    im.save(buf, "PNG", bits=4)
    refused["refused_4bit"] = buf.getvalue()
    laced = ref.random_image(rng, 9, 13, 2)
    refused["refused_adam7"] = ref.encode_adam7(laced, 2)
    for name, data in refused.items():
        depth, ct, _, _, lace = struct.unpack(">BBBBB", dict(ref.chunks(data))[b"IHDR"][8:])
        assert {"refused_16bit": depth == 16, "refused_4bit": depth == 4 and ct == 3, "refused_adam7": lace == 1}[name], name
        d[f"{name}_png"], d[f"{name}_rgb"] = np.frombuffer(data, np.uint8), pillow_decode(data)
    assert np.array_equal(d["refused_adam7_rgb"], laced)
    d["refused"] = np.asarray(list(refused))
    # malformed streams
    good = ref.encode_png(rgb, 2, np.arange(9) % 5)
    bad = {}
    at = good.index(b"IDAT") + 10
    bad["bad_crc"] = good[:at] + bytes([good[at] ^ 1]) + good[at + 1:]
    comp = zlib.compress(ref.filter_rows(rgb, 2, np.arange(9) % 5).tobytes(), 6)
    bad["bad_truncated"] = ref.wrap(13, 9, 2, comp[:len(comp) // 2])
    rows = ref.filter_rows(rgb, 2, np.arange(9) % 5).copy()
    rows[4, 0] = 5
    bad["bad_filter5"] = ref.wrap(13, 9, 2, zlib.compress(rows.tobytes()))
    bad["bad_trailing"] = ref.wrap(13, 9, 2, zlib.compress(ref.filter_rows(ref.random_image(rng, 10, 13, 2), 2, 1).tobytes()))
    for name, data in bad.items():
        d[f"{name}_png"] = np.frombuffer(data, np.uint8)
    d["malformed"] = np.asarray(list(bad))
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(names), "accepted streams")


if __name__ == "__main__":
    main()
