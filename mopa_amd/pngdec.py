"""PNG decoding, split at the filtered scanlines: PNG bytes -> the ``uint8`` ``(H, W, 3)`` image that
``np.asarray(Image.open(...).convert("RGB"))`` returns (Pillow), bit for bit, already on the device and in the layout
``imageprep.resize_bilinear_u8`` / ``imageprep.prepare_batch`` / ``a2d2prep.prepare_frames_a2d2`` read.

Inflate is a serial walk over untrusted bits and runs on the host (the standard library's ``zlib``; the images of a call on a small
thread pool -- ``zlib`` releases the GIL); undoing the per-row filters (None / Sub / Up / Average / Paeth) and the expansion to RGB
run on the device (``csrc/pngdec.hip``): per chunk of up to 32 images ONE asynchronous copy of the headers and filtered scanlines
from one pinned buffer, then ONE launch, no read-back.  There is no CPU fallback for the device half.

Supported: 8-bit samples, colour types 0 (grey), 2 (RGB), 3 (palette), 4 (grey + alpha), 6 (RGBA), non-interlaced, sides 1..8192;
a tRNS chunk is accepted and does not change the pixels.  The result is ``convert("RGB")``: RGB as it is, RGBA without its alpha,
grey replicated to three channels, grey + alpha likewise, palette indices looked up in PLTE (an index past the PLTE length gives
(0, 0, 0)).  16-bit and 1/2/4-bit depths, Adam7 interlace and APNG (``acTL``) raise ``PngUnsupported`` naming the reason; the
caller then decodes that file with Pillow.  A malformed stream (signature, CRC, a missing IHDR / PLTE / IEND, an inflate error,
output shorter or longer than ``H * (1 + stride)``, a filter byte above 4, a zero side) raises ``PngDataError``.  Both are raised
before anything is launched.

Arithmetic: DESIGN.md section 4.  Yardstick: ``tests/_png_reference.py``, held against Pillow 12.2 bit for bit.
"""
from __future__ import annotations

import collections
import ctypes
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import call, chunk_ranges, host_addr, host_ptrs, ptr, stream
from .jpegdec import _bytes_view, _check_out, _pinned, _Staging

_NAME = "pngdec"
DEFAULT_THREADS = 4            # the inflate pool: small and fixed (the loaders' workers already share the host's cores)
MAX_SIDE = 8192
SIGNATURE = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}                      # bytes per pixel of the 8-bit colour types
MODES = {0: "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}      # what Pillow opens them as
_ALIGN = 256                   # of an image's scanlines (and of a chunk's headers) inside the staging buffer


class PngUnsupported(ValueError):
    """A well-formed stream outside the supported subset: decode it with Pillow instead."""


class PngDataError(ValueError):
    """A malformed stream."""


class Header(ctypes.Structure):
    """``PngHeader`` of csrc/pngdec.hip.  ``palette``: R | G << 8 | B << 16 per entry, zero past the PLTE length."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("color_type", ctypes.c_int32), ("bpp", ctypes.c_int32),
                ("palette", ctypes.c_uint32 * 256)]

    @property
    def stride(self):
        """Bytes of a row behind its filter byte."""
        return self.width * self.bpp

    @property
    def scan_bytes(self):
        return self.height * (1 + self.width * self.bpp)


PngInfo = collections.namedtuple("PngInfo", "size mode bit_depth interlaced supported reason")
# size (W, H); mode: what Pillow would open it as ("L", "RGB", "P", "LA", "RGBA"; None for another depth); bit_depth; interlaced: bool;
# supported: bool; reason: None or why not

_Parsed = collections.namedtuple("_Parsed", "width height bit_depth color_type interlace plte idat apng")


def _lib_fn(name):
    return getattr(_lib._lib or _lib.load(), name)


def _check_layout():
    n = _lib_fn("mopa_png_header_bytes")()
    if n != ctypes.sizeof(Header):
        raise RuntimeError(f"{_NAME}: the library's PngHeader has {n} bytes, the binding's {ctypes.sizeof(Header)}")


def _parse(view, who, which=""):
    """The chunk walk: signature, every chunk's CRC32, IHDR first, PLTE / IDAT / IEND; ancillary chunks are skipped."""
    def bad(msg):
        return PngDataError(f"{who}: {which}malformed PNG stream: {msg}")

    data = memoryview(view)
    n = len(data)
    if n < 8 or bytes(data[:8]) != SIGNATURE:
        raise bad("no PNG signature")
    at, ihdr, plte, idat, apng, ended, idat_closed = 8, None, None, [], False, False, False
    while at < n:
        if at + 12 > n:
            raise bad("a chunk is cut off")
        length, = struct.unpack(">I", data[at:at + 4])
        kind = bytes(data[at + 4:at + 8])
        if length > n - at - 12:
            raise bad(f"chunk {kind!r} is cut off")
        body = data[at + 8:at + 8 + length]
        crc, = struct.unpack(">I", data[at + 8 + length:at + 12 + length])
        if zlib.crc32(data[at + 4:at + 8 + length]) != crc:
            raise bad(f"CRC of chunk {kind!r}")
        at += 12 + length
        if ihdr is None and kind != b"IHDR":
            raise bad("the first chunk is not IHDR")
        if kind == b"IHDR":
            if ihdr is not None or length != 13:
                raise bad("IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            if plte is not None or idat or length % 3 or not 3 <= length <= 768:
                raise bad("PLTE")
            plte = bytes(body)
        elif kind == b"IDAT":
            if idat_closed:
                raise bad("IDAT chunks are not consecutive")
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            break
        else:
            if kind == b"acTL":
                apng = True
            elif not kind[0] & 0x20:
                raise bad(f"unknown critical chunk {kind!r}")
        if idat and kind != b"IDAT":
            idat_closed = True
    if ihdr is None:
        raise bad("no IHDR")
    w, h, depth, ct, comp, filt, lace = ihdr
    if w == 0 or h == 0 or w >= 1 << 31 or h >= 1 << 31:
        raise bad(f"sides {w} x {h}")
    if ct not in BPP or depth not in (1, 2, 4, 8, 16) or (ct == 3 and depth == 16) or (ct in (2, 4, 6) and depth < 8):
        raise bad(f"colour type {ct} at bit depth {depth}")
    if comp != 0 or filt != 0 or lace > 1:
        raise bad("compression, filter or interlace method")
    if not ended:
        raise bad("no IEND")
    if not idat:
        raise bad("no IDAT")
    if ct == 3 and plte is None:
        raise bad("no PLTE in front of the image data of a palette image")
    return _Parsed(w, h, depth, ct, lace, plte, idat, apng)


def _reason(p):
    if p.bit_depth != 8:
        return f"{p.bit_depth}-bit samples"
    if p.interlace:
        return "Adam7 interlace"
    if p.apng:
        return "APNG (an acTL chunk)"
    if p.width > MAX_SIDE or p.height > MAX_SIDE:
        return f"a side above {MAX_SIDE}"
    return None


def _header(p, who, which=""):
    why = _reason(p)
    if why is not None:
        raise PngUnsupported(f"{who}: {which}unsupported stream: {why}")
    h = Header()
    h.width, h.height, h.color_type, h.bpp = p.width, p.height, p.color_type, BPP[p.color_type]
    if p.color_type == 3:
        rgb = np.frombuffer(p.plte, np.uint8).reshape(-1, 3).astype(np.uint32)
        np.ctypeslib.as_array(h.palette)[:len(rgb)] = rgb[:, 0] | rgb[:, 1] << 8 | rgb[:, 2] << 16
    return h


def png_info(data) -> PngInfo:
    """Size, mode, depth, interlace and whether ``decode_png_batch`` takes the stream, from its chunks alone (no GPU).  A malformed
    stream raises ``PngDataError``."""
    who = f"{_NAME}.png_info"
    p = _parse(_bytes_view(data, who), who)
    why = _reason(p)
    return PngInfo((p.width, p.height), MODES[p.color_type] if p.bit_depth == 8 else None, p.bit_depth, bool(p.interlace), why is None, why)


def _inflate(p, hdr, who, which=""):
    """-> the ``H * (1 + stride)`` filtered bytes.  The output is capped one byte past what the header promises."""
    need = hdr.scan_bytes
    d = zlib.decompressobj()
    try:
        raw = d.decompress(p.idat[0] if len(p.idat) == 1 else b"".join(p.idat), need + 1)
    except zlib.error as e:
        raise PngDataError(f"{who}: {which}malformed PNG stream: inflate: {e}") from None
    if len(raw) != need:
        raise PngDataError(f"{who}: {which}malformed PNG stream: the image data inflate to {'more' if len(raw) > need else len(raw)} "
                           f"bytes, the header promises {need}")
    if not d.eof:
        raise PngDataError(f"{who}: {which}malformed PNG stream: the image data end inside the compressed stream")
    worst = int(np.frombuffer(raw, np.uint8)[::1 + hdr.stride].max())
    if worst > 4:
        raise PngDataError(f"{who}: {which}malformed PNG stream: filter byte {worst}")
    return raw


def inflate_scanlines(data, out=None):
    """The host half alone: -> (Header, buffer).  ``buffer`` is a 1-D uint8 host tensor (pinned when allocated here and a GPU is
    present) of ``header.scan_bytes`` bytes: per row the filter byte, then the ``stride`` filtered bytes.  ``out``: a contiguous
    uint8 host tensor or numpy array to fill instead (at least ``scan_bytes`` long; the result is its leading slice)."""
    who = f"{_NAME}.inflate_scanlines"
    p = _parse(_bytes_view(data, who), who)
    hdr = _header(p, who)
    need = hdr.scan_bytes
    if out is not None:
        buf = torch.from_numpy(out) if isinstance(out, np.ndarray) else out
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() or buf.is_cuda:
            raise ValueError(f"{who}: out must be a contiguous 1-D uint8 host tensor or array")
        if buf.numel() < need:
            raise ValueError(f"{who}: out holds {buf.numel()} bytes, the scanlines need {need}")
    raw = _inflate(p, hdr, who)
    if out is None:
        buf = _pinned(need) if torch.cuda.is_available() else torch.empty(need, dtype=torch.uint8)
    ctypes.memmove(buf.data_ptr(), raw, need)
    return hdr, buf[:need]


# ------------------------------------------------------------------------------------------------ the device half
def _launch(headers, headers_dev, scan_ptrs, scan_bytes, outs):
    B = len(headers)
    harr = (Header * B)(*headers)
    sb = (ctypes.c_int64 * B)(*scan_bytes)
    pitch = (ctypes.c_int64 * B)(*[t.stride(0) if t.shape[0] > 1 else 3 * t.shape[1] for t in outs])
    sp, dp = host_ptrs(scan_ptrs), host_ptrs(outs)
    call("mopa_png_decode_batch", host_addr(sp), host_addr(sb), ctypes.addressof(harr), headers_dev, B, host_addr(dp), host_addr(pitch),
         stream())


def _header_bytes(headers):
    return np.frombuffer(bytearray((Header * len(headers))(*headers)), np.uint8)


def _device_for(who, out, sizes, device):
    dev = _check_out(who, out, sizes, None if device is None else torch.device(device)) if out is not None else \
        (torch.device("cuda") if device is None else torch.device(device))
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the device half runs on the GPU (there is no CPU fallback), got device {dev}")
    return dev


def decode_scanlines_batch(headers, buffers, out=None, device=None):
    """The device half alone: the headers and filtered scanlines of B images (``inflate_scanlines``, or made by hand) -> a list of
    B (H, W, 3) uint8 device tensors (``out`` if given, filled in place).  ``buffers``: 1-D uint8 host tensors (uploaded here, one
    copy per image) or device tensors, each exactly ``header.scan_bytes`` long."""
    who = f"{_NAME}.decode_scanlines_batch"
    headers, buffers = list(headers), list(buffers)
    if not headers or len(headers) != len(buffers):
        raise ValueError(f"{who}: one buffer per header, and at least one")
    _check_layout()
    for b, (h, t) in enumerate(zip(headers, buffers)):
        if not isinstance(h, Header):
            raise TypeError(f"{who}: headers[{b}] must be a pngdec.Header, got {type(h).__name__}")
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
            raise TypeError(f"{who}: buffers[{b}] must be a contiguous 1-D uint8 tensor")
        if not (1 <= h.width <= MAX_SIDE and 1 <= h.height <= MAX_SIDE) or BPP.get(h.color_type) != h.bpp:
            raise ValueError(f"{who}: headers[{b}] ({h.width} x {h.height}, colour type {h.color_type}, {h.bpp} bytes per pixel) "
                             "is not a supported image")
        if t.numel() != h.scan_bytes:
            raise ValueError(f"{who}: buffers[{b}] holds {t.numel()} bytes, the header's scanlines are {h.scan_bytes}")
    sizes = [(h.width, h.height) for h in headers]
    dev = _device_for(who, out, sizes, device)
    with torch.cuda.device(dev):
        if out is None:
            out = [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for w, h in sizes]
        bufs = [t if t.is_cuda else t.to(dev, non_blocking=True) for t in buffers]
        for s, e in chunk_ranges(len(headers), _lib.query("mopa_png_max_images")):
            hdev = torch.from_numpy(_header_bytes(headers[s:e])).to(dev)
            _launch(headers[s:e], ptr(hdev), [ptr(t) for t in bufs[s:e]], [t.numel() for t in bufs[s:e]], out[s:e])
    return out


_staging = _Staging()
_pools = {}


def _pool(threads):
    p = _pools.get(threads)
    if p is None:
        p = _pools[threads] = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="mopa-png")
    return p


def _up(n):
    return -(-int(n) // _ALIGN) * _ALIGN


def decode_png_batch(datas, out=None, threads=None, device=None):
    """B PNG streams -> a list of B (H, W, 3) uint8 device tensors with the bits of Pillow's ``convert("RGB")`` (images of any sizes
    and colour types in one call).  ``datas``: a list of ``bytes`` / ``memoryview`` / 1-D uint8 arrays (host).  ``out``: a list of B
    uint8 (H, W, 3) device tensors to fill instead, pixels contiguous, rows at any pitch >= 3 W (views of a wider buffer); one that
    overlaps another, or has the wrong shape, dtype or device, is refused.  ``threads``: the size of the inflate pool (default 4;
    1 = the calling thread).

    The chunks of every stream are read first, then all images are inflated (on the pool) into one pinned buffer: ``PngUnsupported``
    (decode that file with Pillow) and ``PngDataError`` are raised before anything is launched.  Then, per chunk of up to 32 images:
    one asynchronous copy of the chunk's headers and scanlines, one launch.  No read-back."""
    who = f"{_NAME}.decode_png_batch"
    if isinstance(datas, (bytes, bytearray, memoryview, np.ndarray, torch.Tensor)):
        raise TypeError(f"{who}: datas must be a list of streams, got one {type(datas).__name__}")
    views = [_bytes_view(d, who, f"datas[{b}]") for b, d in enumerate(datas)]
    if not views:
        raise ValueError(f"{who}: no streams")
    threads = DEFAULT_THREADS if threads is None else int(threads)
    if threads < 1 or threads > 64:
        raise ValueError(f"{who}: threads must be in 1..64, got {threads}")
    _check_layout()
    parsed = [_parse(v, who, f"datas[{b}]: ") for b, v in enumerate(views)]
    headers = [_header(p, who, f"datas[{b}]: ") for b, p in enumerate(parsed)]
    sizes = [(h.width, h.height) for h in headers]
    dev = _device_for(who, out, sizes, device)
    # the staging buffer: per chunk the chunk's headers, then each image's scanlines, all at aligned offsets
    chunks = chunk_ranges(len(views), _lib.query("mopa_png_max_images"))
    offs, bounds, total = [0] * len(views), [], 0
    for s, e in chunks:
        lo = total
        total += _up((e - s) * ctypes.sizeof(Header))
        for b in range(s, e):
            offs[b] = total
            total += _up(headers[b].scan_bytes)
        bounds.append((lo, total))
    with torch.cuda.device(dev):
        stage = _staging.get(total)
        base = stage.data_ptr()

        def inflate(b):
            raw = _inflate(parsed[b], headers[b], who, f"datas[{b}]: ")
            ctypes.memmove(base + offs[b], raw, len(raw))

        if threads == 1 or len(views) == 1:
            for b in range(len(views)):
                inflate(b)
        else:
            futures = [_pool(threads).submit(inflate, b) for b in range(len(views))]
            errors = [f.exception() for f in futures]                   # every thread is out of the buffer before anything is raised
            for e in errors:
                if e is not None:
                    raise e                                             # the first one, in input order
        host = stage.numpy()
        for (s, e), (lo, hi) in zip(chunks, bounds):
            host[lo:lo + (e - s) * ctypes.sizeof(Header)] = _header_bytes(headers[s:e])
        if out is None:
            out = [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for w, h in sizes]
        for (s, e), (lo, hi) in zip(chunks, bounds):
            devbuf = torch.empty(hi - lo, dtype=torch.uint8, device=dev)
            devbuf.copy_(stage[lo:hi], non_blocking=True)
            _launch(headers[s:e], devbuf.data_ptr(), [devbuf.data_ptr() + offs[b] - lo for b in range(s, e)],
                    [headers[b].scan_bytes for b in range(s, e)], out[s:e])
        _staging.fence()
    return list(out)
