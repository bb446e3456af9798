"""A numpy restatement of the baseline JPEG decoding chain that Pillow (libjpeg-turbo, default settings) runs, in its own words:
marker parser -> Huffman decoding -> dequantisation -> the accurate integer inverse DCT -> "fancy" chroma upsampling -> YCbCr to
RGB.  TEST INFRASTRUCTURE ONLY: slow (a Python loop over every Huffman symbol) and plain on purpose.

It is held against Pillow itself by tests/golden_gen/g16_jpegdec.py (which refuses to write otherwise) and by
tests/test_jpegdec_host.py wherever Pillow can be imported; the library (csrc/jpeg_entropy.h, csrc/jpegdec.hip) is held against it
and against the fixture.

The chain, as Pillow on the generating machine confirmed it bit for bit:
  coefficients   per component int16 (blocks_y, blocks_x, 64) in natural order, the grid padded to whole MCUs
  IDCT           13-bit constants, PASS1_BITS = 2, columns then rows, DESCALE rounding, + 128, clamped to 0..255
  upsampling     a chroma plane of real width dw = ceil(W / 2) (and height dh = ceil(H / 2) for 2 x 2):
                   dw <= 2       replication (the library only filters planes wider than two samples)
                   2 x 1         (3 near + far + (1 even | 2 odd)) >> 2, the far column clamped into 0..dw-1
                   2 x 2         s = 3 near_row + far_row (far row clamped into 0..dh-1), then
                                 (3 s[near] + s[far] + (8 even | 7 odd)) >> 4, the far column clamped into 0..dw-1
  colour         R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
                 G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), cb / cr less 128, clamped to 0..255
  one component  replicated to three channels (Image.convert("RGB") of mode L)
"""
import collections

import numpy as np

MAX_SIDE = 8192

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63])


class Unsupported(ValueError):
    """A stream outside the supported subset."""


class DataError(ValueError):
    """A malformed stream."""


Header = collections.namedtuple("Header", "width height ncomp hs vs blocks_x blocks_y comp_w comp_h restart_interval quant")
# hs / vs: the luma sampling factors (chroma is 1 x 1); blocks_* / comp_*: per component; quant: (ncomp, 64) uint16, natural order


# ------------------------------------------------------------------------------------------------ markers
def _u16(data, p):
    if p + 2 > len(data):
        raise DataError("truncated segment")
    return data[p] << 8 | data[p + 1]


def parse_headers(data):
    """Everything in front of the entropy-coded data: -> (Header, Huffman tables, scan component table selectors, position of the
    first entropy-coded byte).  Raises Unsupported / DataError."""
    data = bytes(data)
    if len(data) < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise DataError("no SOI")
    p = 2
    qt, huff, frame, ri = {}, {}, None, 0
    jfif, adobe = False, None
    while True:
        if p >= len(data):
            raise DataError("the stream ends in front of SOS")
        if data[p] != 0xFF:
            raise DataError("a marker was expected")
        while p < len(data) and data[p] == 0xFF:
            p += 1
        if p >= len(data):
            raise DataError("the stream ends in a marker")
        m = data[p]
        p += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            raise DataError(f"marker FF{m:02X} in front of SOS")
        if m == 0xD9:
            raise DataError("EOI in front of SOS")
        if m == 0x00:
            raise DataError("a stuffed byte outside entropy-coded data")
        n = _u16(data, p)
        if n < 2 or p + n > len(data):
            raise DataError("truncated segment")
        seg = data[p + 2:p + n]
        p += n
        if m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Unsupported({0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless"}.get(m, "arithmetic or differential") + " JPEG")
        if m == 0xC0:
            if frame is not None:
                raise DataError("two frames")
            if len(seg) < 6:
                raise DataError("truncated SOF0")
            prec, h, w, nc = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            if len(seg) != 6 + 3 * nc:
                raise DataError("SOF0 of the wrong length")
            if prec != 8:
                raise Unsupported(f"{prec}-bit samples")
            if w == 0 or h == 0:
                raise DataError("empty image")
            if nc not in (1, 3):
                raise Unsupported(f"{nc} components")
            if w > MAX_SIDE or h > MAX_SIDE:
                raise Unsupported(f"image larger than {MAX_SIDE} on a side")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
            if nc == 1:
                comps = [(comps[0][0], 1, 1, comps[0][3])]        # the factors of a single component do not matter
            else:
                if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                    raise Unsupported("sampling factors " + ", ".join(f"{c[1]}x{c[2]}" for c in comps))
            if any(c[3] > 3 for c in comps):
                raise DataError("quantisation table selector above 3")
            frame = (w, h, comps)
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq > 1 or tq > 3:
                    raise DataError("bad DQT")
                size = 64 * (pq + 1)
                if q + 1 + size > len(seg):
                    raise DataError("truncated DQT")
                raw = seg[q + 1:q + 1 + size]
                vals = [raw[2 * k] << 8 | raw[2 * k + 1] for k in range(64)] if pq else list(raw)
                nat = np.zeros(64, np.uint16)
                nat[ZIGZAG] = vals
                qt[tq] = nat
                q += 1 + size
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise DataError("truncated DHT")
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or q + 17 + total > len(seg):
                    raise DataError("bad DHT")
                huff[(tc, th)] = _huff_table(counts, list(seg[q + 17:q + 17 + total]), tc)
                q += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                raise DataError("bad DRI")
            ri = seg[0] << 8 | seg[1]
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            if seg[:5] == b"Adobe" and len(seg) >= 12:
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise DataError("SOS in front of SOF")
            w, h, comps = frame
            nc = len(comps)
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                raise DataError("SOS of the wrong length")
            if seg[0] != nc:
                raise Unsupported("more than one scan")
            sel = []
            for i in range(nc):
                if seg[1 + 2 * i] != comps[i][0]:
                    raise Unsupported("scan components out of frame order")
                sel.append((seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15))
            ss, se, ahl = seg[1 + 2 * nc:4 + 2 * nc]
            if (ss, se, ahl) != (0, 63, 0):
                raise Unsupported("spectral selection or successive approximation in a sequential frame")
            if nc == 3 and not jfif:
                if adobe is not None and adobe != 1:
                    raise Unsupported(f"Adobe transform {adobe} (not YCbCr)")
                if adobe is None and [c[0] for c in comps] == [82, 71, 66]:
                    raise Unsupported("components named R, G, B (not YCbCr)")
            for i, (td, ta) in enumerate(sel):
                if td > 3 or ta > 3 or (0, td) not in huff or (1, ta) not in huff:
                    raise DataError("the scan names a Huffman table that was not defined")
                if comps[i][3] not in qt:
                    raise DataError("the frame names a quantisation table that was not defined")
            hs, vs = comps[0][1], comps[0][2]
            mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
            bx = [mx * hs] + [mx] * (nc - 1)
            by = [my * vs] + [my] * (nc - 1)
            cw = [w] + [-(-w // hs)] * (nc - 1)
            ch = [h] + [-(-h // vs)] * (nc - 1)
            hdr = Header(w, h, nc, hs, vs, tuple(bx), tuple(by), tuple(cw), tuple(ch), ri, np.stack([qt[c[3]] for c in comps]))
            return hdr, [(huff[(0, td)], huff[(1, ta)]) for td, ta in sel], p
        # APPn, COM and anything else with a length: skipped


def _huff_table(counts, vals, tc):
    """code length and value by (length, code)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= 1 << length:
                raise DataError("over-subscribed Huffman table")
            if tc == 0 and vals[k] > 15:
                raise DataError("DC category above 15")
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


# ------------------------------------------------------------------------------------------------ entropy-coded data
class _Bits:
    def __init__(self, data, p):
        self.d, self.p, self.acc, self.n = data, p, 0, 0

    def _byte(self):
        d, p = self.d, self.p
        if p >= len(d):
            raise DataError("the stream ends inside the entropy-coded data")
        b = d[p]
        if b == 0xFF:
            if p + 1 >= len(d):
                raise DataError("the stream ends inside the entropy-coded data")
            if d[p + 1] != 0:
                raise DataError("a marker inside an entropy-coded segment")
            p += 1
        self.p = p + 1
        return b

    def bit(self):
        if self.n == 0:
            self.acc, self.n = self._byte(), 8
        self.n -= 1
        return self.acc >> self.n & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = v << 1 | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise DataError("a Huffman code that is not in the table")

    def marker(self):
        """Drop the rest of the byte, skip fill bytes, -> the marker code (consumed)."""
        self.n = 0
        d, p = self.d, self.p
        if p >= len(d) or d[p] != 0xFF:
            raise DataError("a marker was expected")
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise DataError("the stream ends in a marker")
        self.p = p + 1
        return d[p]


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < 1 << (s - 1) else v


def decode_coefficients(data):
    """-> (Header, [per component int16 (blocks_y, blocks_x, 64), natural order, quantised])."""
    data = bytes(data)
    hdr, tabs, p = parse_headers(data)
    planes = [np.zeros((hdr.blocks_y[c], hdr.blocks_x[c], 64), np.int16) for c in range(hdr.ncomp)]
    br = _Bits(data, p)
    mx, my = hdr.blocks_x[-1] if hdr.ncomp == 3 else hdr.blocks_x[0], hdr.blocks_y[-1] if hdr.ncomp == 3 else hdr.blocks_y[0]
    shape = [(hdr.hs, hdr.vs)] + [(1, 1)] * (hdr.ncomp - 1)
    pred = [0] * hdr.ncomp
    total, rst = mx * my, 0
    for mcu in range(total):
        if hdr.restart_interval and mcu and mcu % hdr.restart_interval == 0:
            if br.marker() != 0xD0 + (rst & 7):
                raise DataError("a missing or out-of-order restart marker")
            rst += 1
            pred = [0] * hdr.ncomp
        my_, mx_ = divmod(mcu, mx)
        for c in range(hdr.ncomp):
            dc, ac = tabs[c]
            for v in range(shape[c][1]):
                for h in range(shape[c][0]):
                    blk = planes[c][my_ * shape[c][1] + v, mx_ * shape[c][0] + h]
                    s = br.symbol(dc)
                    pred[c] += _extend(br.bits(s), s)
                    blk[0] = np.int16(((pred[c] + 32768) & 65535) - 32768)
                    k = 1
                    while k < 64:
                        rs = br.symbol(ac)
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            raise DataError("a run past coefficient 63")
                        blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                        k += 1
    if br.marker() != 0xD9:
        raise DataError("no EOI after the scan")
    return hdr, planes


# ------------------------------------------------------------------------------------------------ inverse DCT
_C = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
          f2562=20995, f3072=25172)


def _idct_1d(x, shift):
    """x: (..., 8) int64 along the last axis -> (..., 8), descaled by `shift` with rounding."""
    c = _C
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * c["f0541"]
    t2 = z1 - z3 * c["f1847"]
    t3 = z1 + z2 * c["f0765"]
    t0 = (x[..., 0] + x[..., 4]) << 13
    t1 = (x[..., 0] - x[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * c["f1175"]
    t0, t1, t2, t3 = t0 * c["f0298"], t1 * c["f2053"], t2 * c["f3072"], t3 * c["f1501"]
    z1, z2 = -z1 * c["f0899"], -z2 * c["f2562"]
    z3, z4 = -z3 * c["f1961"] + z5, -z4 * c["f0390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct_plane(coeff, quant):
    """coeff: (by, bx, 64) int16, quant: (64,) -> (by * 8, bx * 8) uint8."""
    by, bx, _ = coeff.shape
    x = (coeff.astype(np.int64) * quant.astype(np.int64)).reshape(by, bx, 8, 8)
    ws = _idct_1d(x.swapaxes(2, 3), 11).swapaxes(2, 3)            # pass 1 walks the columns
    px = _idct_1d(ws, 18) + 128                                   # pass 2 the rows
    return np.clip(px, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


# ------------------------------------------------------------------------------------------------ upsampling and colour
def upsample(plane, hs, vs, dw, dh, W, H):
    """plane: the padded component plane, of which (dh, dw) is real -> (H, W) int32 at full resolution."""
    p = plane[:dh, :dw].astype(np.int32)
    if hs == 1 and vs == 1:
        return p[:H, :W]
    x, y = np.arange(W), np.arange(H)
    if dw <= 2:
        return p[(y >> 1 if vs == 2 else y)[:, None], (x >> 1)[None, :]]
    near_x = x >> 1
    far_x = np.clip(np.where(x & 1, near_x + 1, near_x - 1), 0, dw - 1)
    if vs == 1:
        return (3 * p[:, near_x] + p[:, far_x] + np.where(x & 1, 2, 1)[None, :])[:H] >> 2
    near_y = y >> 1
    far_y = np.clip(np.where(y & 1, near_y + 1, near_y - 1), 0, dh - 1)
    s = 3 * p[near_y] + p[far_y]
    return (3 * s[:, near_x] + s[:, far_x] + np.where(x & 1, 7, 8)[None, :]) >> 4


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def component_planes(hdr, planes):
    return [idct_plane(planes[c], hdr.quant[c]) for c in range(hdr.ncomp)]


def pixels(hdr, comp):
    """The uint8 component planes -> (H, W, 3) uint8."""
    W, H = hdr.width, hdr.height
    y = comp[0][:H, :W].astype(np.int32)
    if hdr.ncomp == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, 2)
    cb, cr = (upsample(comp[c], hdr.hs, hdr.vs, hdr.comp_w[c], hdr.comp_h[c], W, H) for c in (1, 2))
    return ycc_to_rgb(y, cb, cr)


def decode(data):
    """JPEG bytes -> (H, W, 3) uint8, what np.asarray(Image.open(...).convert("RGB")) gives."""
    hdr, planes = decode_coefficients(data)
    return pixels(hdr, component_planes(hdr, planes))


# ------------------------------------------------------------------------------------------------ the fixture's cases
SAMPLINGS = {"444": 0, "422": 1, "420": 2}          # Pillow's `subsampling` argument


def synthetic(W, H, seed, gray=False):
    """Smooth content plus noise, so that chroma edges exist."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = []
    for k in range(1 if gray else 3):
        f = 0.05 + 0.07 * k
        ch.append(128 + 90 * np.sin(f * xx + 0.6 * k) * np.cos((f + 0.03) * yy + 0.3 * k) + rng.normal(0, 18, (H, W)))
    img = np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)
    return img[:, :, 0] if gray else img


def small_cases():
    """[(name, W, H, sampling name | None for grey, encoder options)]: every width of WS and every height of HS with every sampling,
    the qualities, optimised tables, restart intervals, a grey image and a 40 x 56 image per sampling."""
    WS, HS = (1, 7, 8, 9, 15, 16, 17, 33), (1, 8, 9, 16, 17)
    out = []
    for s in SAMPLINGS:
        for i, w in enumerate(WS):                  # every width; the heights rotate
            out.append((f"s{s}_{w}x{HS[i % 5]}", w, HS[i % 5], s, dict(quality=75)))
        for w, h in ((33, 1), (17, 9), (9, 17), (1, 16), (15, 8), (16, 17), (7, 9)):      # every height again, other pairings
            if not any(c[1] == w and c[2] == h and c[3] == s for c in out):
                out.append((f"s{s}_{w}x{h}", w, h, s, dict(quality=75)))
        out.append((f"s{s}_q10", 33, 17, s, dict(quality=10)))
        out.append((f"s{s}_q100", 17, 16, s, dict(quality=100)))
        out.append((f"s{s}_opt", 33, 17, s, dict(quality=75, optimize=True)))
        out.append((f"s{s}_rst1", 33, 17, s, dict(quality=75, restart_marker_blocks=1)))
        out.append((f"s{s}_rst3", 33, 17, s, dict(quality=75, restart_marker_blocks=3)))
        out.append((f"s{s}_40x56", 40, 56, s, dict(quality=90)))
    out.append(("grey_33x17", 33, 17, None, dict(quality=75)))
    return out
