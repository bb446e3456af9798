"""Generate tests/golden/g16_jpegdec.npz and g16_jpegdec_fullsize.json by RUNNING Pillow (libjpeg-turbo): synthetic images are
encoded by Pillow and decoded by Pillow (``np.asarray(Image.open(...).convert("RGB"))``).

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixture is what travels).
Usage, from the repo root:  python tests/golden_gen/g16_jpegdec.py

Refuses to write unless the numpy restatement tests/_jpeg_reference.py equals Pillow on every case, the full-size one included.

Contents of the npz:
  names                      the small cases (tests/_jpeg_reference.py::small_cases), in order
  <name>_jpg                 the stream, uint8
  <name>_rgb                 Pillow's decoded (H, W, 3) uint8 array
  <name>_c0 [_c1, _c2]       the restatement's quantised coefficient planes, int16 (blocks_y, blocks_x, 64), natural order
  <name>_quant               (ncomp, 64) uint16, natural order
  <name>_geom                int32 [W, H, ncomp, hs, vs, restart interval]
  refused_progressive_jpg, refused_1x2_jpg   streams the library must refuse (the second is a 4:4:4 stream whose frame header
                             was rewritten to 1 x 2 luma sampling: only its headers are ever read)
  full_jpg                   one 1600 x 900 4:2:0 stream at quality 75
The json: size, CRC32 and byte sum of Pillow's decode of full_jpg.
"""
import io
import json
import os
import sys
import zlib

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jpeg_reference as ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g16_jpegdec.npz")
OUT_FULL = os.path.join(ROOT, "tests", "golden", "g16_jpegdec_fullsize.json")
LARGEST_COMMITTED = 807257          # g12_minent.npz


def encode(img, sampling, **opts):
    buf = io.BytesIO()
    if sampling is not None:
        opts["subsampling"] = ref.SAMPLINGS[sampling]
    Image.fromarray(img).save(buf, "JPEG", **opts)
    return buf.getvalue()


def pillow_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def checked(name, data):
    want = pillow_decode(data)
    hdr, planes = ref.decode_coefficients(data)
    got = ref.pixels(hdr, ref.component_planes(hdr, planes))
    if got.shape != want.shape or not np.array_equal(got, want):
        bad = int((got != want).sum()) if got.shape == want.shape else -1
        raise SystemExit(f"the restatement differs from Pillow on {name} ({bad} bytes): nothing written")
    return want, hdr, planes


def full_image():
    rng = np.random.Generator(np.random.PCG64(16))
    yy, xx = np.mgrid[0:900, 0:1600].astype(np.float64)
    ch = [128 + 80 * np.sin(0.011 * (k + 1) * xx + k) * np.cos(0.017 * (k + 1) * yy) + rng.normal(0, 6, (900, 1600)) for k in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def main():
    d, names = {}, []
    for k, (name, W, H, sampling, opts) in enumerate(ref.small_cases()):
        img = ref.synthetic(W, H, 1600 + k, gray=sampling is None)
        data = encode(img, sampling, **opts)
        want, hdr, planes = checked(name, data)
        assert (hdr.width, hdr.height) == (W, H) and hdr.ncomp == (1 if sampling is None else 3)
        if sampling is not None:
            assert (hdr.hs, hdr.vs) == {"444": (1, 1), "422": (2, 1), "420": (2, 2)}[sampling], name
        if "restart_marker_blocks" in opts:
            assert hdr.restart_interval == opts["restart_marker_blocks"], name
        names.append(name)
        d[f"{name}_jpg"], d[f"{name}_rgb"] = np.frombuffer(data, np.uint8), want
        for c, p in enumerate(planes):
            d[f"{name}_c{c}"] = p
        d[f"{name}_quant"] = hdr.quant
        d[f"{name}_geom"] = np.asarray([W, H, hdr.ncomp, hdr.hs, hdr.vs, hdr.restart_interval], np.int32)
    d["names"] = np.asarray(names)
    # every width and every height with every sampling
    for s in ref.SAMPLINGS:
        ws = {c[1] for c in ref.small_cases() if c[3] == s}
        hs = {c[2] for c in ref.small_cases() if c[3] == s}
        assert ws >= {1, 7, 8, 9, 15, 16, 17, 33} and hs >= {1, 8, 9, 16, 17}, (s, ws, hs)
    # the quality-100 tables are ones; the optimised streams carry other Huffman tables than the default ones
    assert all((d[f"s{s}_q100_quant"] == 1).all() for s in ref.SAMPLINGS)
    # refused streams
    base = ref.synthetic(33, 17, 99)
    prog = encode(base, "420", quality=75, progressive=True)
    plain = bytearray(encode(base, "444", quality=75))
    at = plain.index(b"\xff\xc0")
    assert plain[at + 11] == 0x11
    plain[at + 11] = 0x12
    for name, data in (("refused_progressive", prog), ("refused_1x2", bytes(plain))):
        try:
            ref.parse_headers(data)
        except ref.Unsupported:
            pass
        else:
            raise SystemExit(f"the restatement accepts {name}: nothing written")
        d[f"{name}_jpg"] = np.frombuffer(data, np.uint8)
    # full size
    data = encode(full_image(), "420", quality=75)
    want, hdr, _ = checked("full size", data)
    d["full_jpg"] = np.frombuffer(data, np.uint8)
    full = {"size": [hdr.width, hdr.height], "sampling": "420", "quality": 75, "stream_bytes": len(data),
            "crc32": zlib.crc32(want.tobytes()), "sum": int(want.sum(dtype=np.uint64))}
    np.savez_compressed(OUT, **d)
    if os.path.getsize(OUT) >= LARGEST_COMMITTED:
        os.remove(OUT)
        raise SystemExit("the fixture would be the largest committed one: nothing kept")
    with open(OUT_FULL, "w") as f:
        json.dump(full, f, indent=1)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(names), "small cases; full-size stream", len(data), "bytes")


if __name__ == "__main__":
    main()
