"""The PNG yardstick in numpy: an encoder whose per-row filter choice the caller forces, a serial decoder for small images, and
the expansion to what Pillow's ``convert("RGB")`` returns.  PNG is lossless, so the expected output of any encoded image is
``expand_rgb(original)``; the fixture tests/golden/g18_pngdec.npz (tests/golden_gen/g18_pngdec.py, which ran Pillow) pins that rule.

Filtered scanlines: per row one filter byte (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth), then ``W * bpp`` bytes; byte i of row y is
the original minus a prediction from the ORIGINAL neighbours a = (y, i - bpp), b = (y - 1, i), c = (y - 1, i - bpp) (zero outside
the image), modulo 256.  Encoding therefore vectorises fully; decoding is a serial recurrence."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
COLOR_TYPES = (0, 2, 3, 4, 6)


def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def as_pixels(img, color_type):
    """(H, W) or (H, W, bpp) uint8 -> (H, W, bpp)."""
    a = np.asarray(img, np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    assert a.ndim == 3 and a.shape[2] == BPP[color_type], (a.shape, color_type)
    return a


def _paeth(a, b, c):
    """int arrays -> the Paeth predictor (ties: a, then b)."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img, color_type, filters):
    """The filtered scanlines of an image: (H, 1 + W * bpp) uint8.  ``filters``: one int for every row, or H of them."""
    px = as_pixels(img, color_type)
    H, W, bpp = px.shape
    f = np.broadcast_to(np.asarray(filters, np.int64), (H,))
    assert ((f >= 0) & (f <= 4)).all()
    x = px.reshape(H, W * bpp).astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    pred = np.stack([np.zeros_like(x), a, b, (a + b) >> 1, _paeth(a, b, c)])[f, np.arange(H)]
    out = np.empty((H, 1 + W * bpp), np.uint8)
    out[:, 0] = f
    out[:, 1:] = (x - pred) & 255
    return out


def ihdr(W, H, color_type, bit_depth=8, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bit_depth, color_type, 0, 0, interlace))


def wrap(W, H, color_type, compressed, palette=None, trns=None, idat_split=1, extra_chunks=(), bit_depth=8, interlace=0):
    """A PNG stream around an already compressed image data stream.  ``idat_split``: how many IDAT chunks (a list gives the byte
    positions to cut at, so that an empty chunk can be asked for).  ``extra_chunks``: (kind, body) pairs put between IHDR and
    PLTE / IDAT."""
    parts = [SIGNATURE, ihdr(W, H, color_type, bit_depth, interlace)]
    parts += [chunk(k, b) for k, b in extra_chunks]
    if palette is not None:
        parts.append(chunk(b"PLTE", np.asarray(palette, np.uint8).reshape(-1, 3).tobytes()))
    if trns is not None:
        parts.append(chunk(b"tRNS", bytes(trns)))
    cuts = list(idat_split) if not isinstance(idat_split, int) else [len(compressed) * k // idat_split for k in range(1, idat_split)]
    cuts = [0] + cuts + [len(compressed)]
    parts += [chunk(b"IDAT", compressed[s:e]) for s, e in zip(cuts[:-1], cuts[1:])]
    parts.append(chunk(b"IEND"))
    return b"".join(parts)


def encode_png(img, color_type, filters, palette=None, trns=None, idat_split=1, level=6, extra_chunks=()):
    """An 8-bit non-interlaced PNG stream of ``img`` ((H, W) or (H, W, bpp) uint8) whose row y uses filter ``filters[y]``."""
    px = as_pixels(img, color_type)
    H, W, _ = px.shape
    if color_type == 3:
        assert palette is not None
    return wrap(W, H, color_type, zlib.compress(filter_rows(px, color_type, filters).tobytes(), level), palette, trns, idat_split,
                extra_chunks)


ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))    # x0, y0, dx, dy


def encode_adam7(img, color_type, palette=None):
    """An Adam7-interlaced stream (every reduced image filtered with None): one the library must refuse and Pillow decodes."""
    px = as_pixels(img, color_type)
    H, W, _ = px.shape
    raw = b""
    for x0, y0, dx, dy in ADAM7:
        sub = px[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            raw += filter_rows(sub, color_type, 0).tobytes()
    return wrap(W, H, color_type, zlib.compress(raw), palette, interlace=1)


def chunks(data):
    """[(kind, body)] of a stream (CRCs checked)."""
    assert data[:8] == SIGNATURE
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert zlib.crc32(kind + body) == struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0], kind
        out.append((kind, body))
        at += 12 + n
        if kind == b"IEND":
            break
    return out


def scanlines(data):
    """-> (W, H, color_type, palette or None, (H, 1 + W * bpp) uint8 filtered scanlines) of an 8-bit non-interlaced stream."""
    cs = chunks(data)
    W, H, depth, ct, _, _, lace = struct.unpack(">IIBBBBB", dict(cs)[b"IHDR"])
    assert depth == 8 and lace == 0 and ct in BPP
    raw = zlib.decompress(b"".join(b for k, b in cs if k == b"IDAT"))
    pal = None
    if ct == 3:
        pal = np.zeros((256, 3), np.uint8)
        p = np.frombuffer(dict(cs)[b"PLTE"], np.uint8).reshape(-1, 3)
        pal[:len(p)] = p
    return W, H, ct, pal, np.frombuffer(raw, np.uint8).reshape(H, 1 + W * BPP[ct])


def unfilter(rows, bpp):
    """(H, 1 + stride) filtered scanlines -> (H, stride) uint8.  Serial: for small images."""
    H, stride = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((H + 1, stride + bpp), np.int64)              # a zero row above, bpp zero bytes to the left
    for y in range(H):
        f, line, prev, cur = int(rows[y, 0]), rows[y, 1:].astype(np.int64), out[y], out[y + 1]
        assert f <= 4
        if f == 0:
            cur[bpp:] = line
        elif f == 2:
            cur[bpp:] = (line + prev[bpp:]) & 255
        else:
            for i in range(stride):
                a, b, c = int(cur[i]), int(prev[i + bpp]), int(prev[i])
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i + bpp] = (int(line[i]) + p) & 255
    return out[1:, bpp:].astype(np.uint8)


def decode_png(data):
    """-> (pixels (H, W, bpp) uint8, color_type, palette (256, 3) zero-filled or None)."""
    W, H, ct, pal, rows = scanlines(data)
    return unfilter(rows, BPP[ct]).reshape(H, W, BPP[ct]), ct, pal


def expand_rgb(pixels, color_type, palette=None):
    """What ``Image.open(...).convert("RGB")`` returns: RGB as it is, RGBA without alpha, grey (and grey + alpha) replicated,
    palette indices looked up (entries past the palette's length are zero)."""
    px = as_pixels(pixels, color_type)
    if color_type in (2, 6):
        return np.ascontiguousarray(px[:, :, :3])
    if color_type == 3:
        pal = np.zeros((256, 3), np.uint8)
        p = np.asarray(palette, np.uint8).reshape(-1, 3)
        pal[:len(p)] = p
        return pal[px[:, :, 0]]
    return np.repeat(px[:, :, :1], 3, axis=2)


def header_for(pd, W, H, color_type, palette=None):
    """A mopa_amd.pngdec.Header for hand-made scanlines."""
    h = pd.Header()
    h.width, h.height, h.color_type, h.bpp = W, H, color_type, BPP[color_type]
    if palette is not None:
        p = np.asarray(palette, np.uint8).reshape(-1, 3).astype(np.uint32)
        np.ctypeslib.as_array(h.palette)[:len(p)] = p[:, 0] | p[:, 1] << 8 | p[:, 2] << 16
    return h


def random_image(rng, H, W, color_type):
    return rng.integers(0, 256, (H, W, BPP[color_type]), dtype=np.uint8)


def synthetic_rgb(H, W, seed):
    """The measurement's image: sinusoids plus Gaussian noise of sigma 6 (compresses to about 0.65 of raw)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = [128 + 80 * np.sin(0.011 * (k + 1) * xx + k) * np.cos(0.017 * (k + 1) * yy) + rng.normal(0, 6, (H, W)) for k in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
