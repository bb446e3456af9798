"""JPEG decoding, split at the quantised coefficients: JPEG bytes -> the ``uint8`` ``(H, W, 3)`` image that
``np.asarray(Image.open(...).convert("RGB"))`` returns (Pillow on libjpeg-turbo, default settings), bit for bit, already on the
device and in the layout ``imageprep.resize_bilinear_u8`` / ``imageprep.prepare_batch`` read.

The Huffman stage is a serial walk over untrusted bits and runs on the host (``csrc/jpeg_entropy.h``, plain C++; the images of a call
on a small thread pool -- ``ctypes`` releases the GIL); dequantisation, the inverse DCT, chroma upsampling and the colour conversion
run on the device (``csrc/jpegdec.hip``): per chunk of up to 32 images ONE asynchronous copy of the coefficients from one pinned
buffer, then ONE launch, no read-back.  There is no CPU fallback for the device half.

Supported: baseline sequential streams, 8-bit, one component (replicated to three channels) or three with chroma at 1 x 1 and luma at
1 x 1, 2 x 1 or 2 x 2 (4:4:4, 4:2:2, 4:2:0), one interleaved scan, restart intervals, default or optimised Huffman tables, sides up
to 8192.  Everything else (progressive, arithmetic, 12-bit, lossless, other sampling factors, four components, an Adobe segment
whose transform is not YCbCr, several scans) raises ``JpegUnsupported`` naming the reason; the caller then decodes that file with
Pillow.  A malformed stream raises ``JpegDataError``.  Both are raised before anything is launched.

Arithmetic: DESIGN.md section 4.  Yardstick: ``tests/_jpeg_reference.py``, held against Pillow 12.2 / libjpeg-turbo bit for bit.
"""
from __future__ import annotations

import collections
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import call, chunk_ranges, host_addr, host_ptrs, ptr, stream

_NAME = "jpegdec"
DEFAULT_THREADS = 4            # the entropy stage's pool: small and fixed (the loaders' workers already share the host's cores)
MAX_SIDE = 8192
ERR_UNSUPPORTED, ERR_DATA = -4, -5
REASONS = {1: "progressive JPEG", 2: "extended sequential, lossless, arithmetic or differential coding", 3: "not 8-bit samples",
           4: "neither 1 nor 3 components", 5: "sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0",
           6: "the colour space is not YCbCr (Adobe transform flag, or components named R, G, B)",
           7: "more than one scan", 8: f"a side above {MAX_SIDE}"}
_ALIGN = 256                   # of an image's coefficients inside a chunk's buffer


class JpegUnsupported(ValueError):
    """A well-formed stream outside the supported subset: decode it with Pillow instead."""


class JpegDataError(ValueError):
    """A malformed stream."""


class Header(ctypes.Structure):
    """``JpegHeader`` of csrc/jpeg_entropy.h."""
    _fields_ = [("plane_off", ctypes.c_int64 * 3), ("coeff_bytes", ctypes.c_int64),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32),
                ("hs", ctypes.c_int32), ("vs", ctypes.c_int32), ("mcus_x", ctypes.c_int32), ("mcus_y", ctypes.c_int32),
                ("blocks_x", ctypes.c_int32 * 3), ("blocks_y", ctypes.c_int32 * 3),
                ("comp_w", ctypes.c_int32 * 3), ("comp_h", ctypes.c_int32 * 3),
                ("restart_interval", ctypes.c_int32), ("supported", ctypes.c_int32), ("reason", ctypes.c_int32),
                ("quant", (ctypes.c_uint16 * 64) * 3)]

    def quant_tables(self) -> np.ndarray:
        """(ncomp, 64) uint16, natural order."""
        return np.ctypeslib.as_array(self.quant)[:self.ncomp].copy()


JpegInfo = collections.namedtuple("JpegInfo", "size mode sampling supported reason")
# size (W, H); mode "L" / "RGB" (what Pillow would open it as: a YCbCr stream converted); sampling "4:4:4" / "4:2:2" / "4:2:0" /
# None (one component, or unknown); supported: bool; reason: None or why not


def _lib_fn(name):
    return getattr(_lib._lib or _lib.load(), name)


def _check_layout():
    n = _lib_fn("mopa_jpeg_header_bytes")()
    if n != ctypes.sizeof(Header):
        raise RuntimeError(f"{_NAME}: the library's JpegHeader has {n} bytes, the binding's {ctypes.sizeof(Header)}")


def _bytes_view(data, who, what="data"):
    """bytes / bytearray / memoryview / uint8 numpy array / uint8 CPU tensor -> a contiguous uint8 numpy view (no copy)."""
    if isinstance(data, torch.Tensor):
        if data.is_cuda:
            raise TypeError(f"{who}: {what} must be host bytes (the entropy stage runs on the host), got a tensor on {data.device}")
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise TypeError(f"{who}: {what} must be bytes or a 1-D uint8 array, got {data.dtype} {tuple(data.shape)}")
        return np.ascontiguousarray(data.numpy())
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise TypeError(f"{who}: {what} must be bytes or a 1-D uint8 array, got {data.dtype} {data.shape}")
        return np.ascontiguousarray(data)
    if isinstance(data, (bytes, bytearray, memoryview)):
        try:
            return np.frombuffer(data, dtype=np.uint8)
        except (ValueError, BufferError):
            raise TypeError(f"{who}: {what} must be a contiguous buffer of bytes") from None
    raise TypeError(f"{who}: {what} must be bytes, a memoryview or a 1-D uint8 array, got {type(data).__name__}")


def _raise_for(rc, hdr, who, which=""):
    if rc == ERR_UNSUPPORTED:
        raise JpegUnsupported(f"{who}: {which}unsupported stream: {REASONS.get(hdr.reason, 'reason %d' % hdr.reason)}")
    if rc == ERR_DATA:
        raise JpegDataError(f"{who}: {which}malformed JPEG stream")
    if rc != 0:
        raise RuntimeError(f"{who}: {which}the entropy stage failed with code {rc}")


def _info(view, who, which=""):
    _check_layout()
    hdr = Header()
    rc = _lib_fn("mopa_jpeg_info")(view.ctypes.data, ctypes.addressof(hdr), view.size)
    if rc not in (0, ERR_UNSUPPORTED):
        _raise_for(rc, hdr, who, which)
    return rc, hdr


def jpeg_info(data) -> JpegInfo:
    """Size, mode, sampling and whether ``decode_jpeg_batch`` takes the stream, from its markers alone (no GPU).  A malformed header
    raises ``JpegDataError``."""
    who = f"{_NAME}.jpeg_info"
    rc, h = _info(_bytes_view(data, who), who)
    sampling = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}.get((h.hs, h.vs)) if h.ncomp == 3 and rc == 0 else None
    mode = {1: "L", 3: "RGB", 4: "CMYK"}.get(h.ncomp)
    return JpegInfo((h.width, h.height), mode, sampling, rc == 0, None if rc == 0 else REASONS.get(h.reason, f"reason {h.reason}"))


def _pinned(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, pin_memory=True)


def decode_entropy(data, out=None):
    """The host half alone: -> (Header, buffer).  ``buffer`` is a 1-D uint8 host tensor (pinned when allocated here and a GPU is
    present) of ``header.coeff_bytes`` bytes: the three quantisation tables (uint16 [3][64], natural order), then per component the
    quantised coefficients int16 [blocks_y][blocks_x][64] in natural order at ``header.plane_off[c]``.  ``out``: a contiguous uint8
    host tensor or numpy array to fill instead (at least ``coeff_bytes`` long; the result is its leading slice)."""
    who = f"{_NAME}.decode_entropy"
    view = _bytes_view(data, who)
    rc, hdr = _info(view, who)
    _raise_for(rc, hdr, who)
    need = int(hdr.coeff_bytes)
    if out is None:
        buf = _pinned(need) if torch.cuda.is_available() else torch.empty(need, dtype=torch.uint8)
    else:
        buf = torch.from_numpy(out) if isinstance(out, np.ndarray) else out
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() or buf.is_cuda:
            raise ValueError(f"{who}: out must be a contiguous 1-D uint8 host tensor or array")
        if buf.numel() < need:
            raise ValueError(f"{who}: out holds {buf.numel()} bytes, the coefficients need {need}")
    rc = _lib_fn("mopa_jpeg_entropy_decode")(view.ctypes.data, ctypes.addressof(hdr), buf.data_ptr(), view.size, buf.numel())
    _raise_for(rc, hdr, who)
    return hdr, buf[:need]


def coefficient_planes(hdr, buf):
    """Views of a ``decode_entropy`` buffer: [per component int16 (blocks_y, blocks_x, 64)]."""
    a = buf.numpy() if isinstance(buf, torch.Tensor) else buf
    return [a[hdr.plane_off[c]:hdr.plane_off[c] + hdr.blocks_x[c] * hdr.blocks_y[c] * 128].view(np.int16)
            .reshape(hdr.blocks_y[c], hdr.blocks_x[c], 64) for c in range(hdr.ncomp)]


def pack_coefficients(size, planes, quant, sampling=None):
    """The inverse, for feeding the device half with coefficients from elsewhere: ``size`` (W, H), ``planes`` [per component int16
    (blocks_y, blocks_x, 64)], ``quant`` (ncomp, 64) uint16, ``sampling`` the luma factors (hs, vs) (default (1, 1)) -> (Header,
    1-D uint8 host tensor)."""
    who = f"{_NAME}.pack_coefficients"
    _check_layout()
    hdr = Header()
    hdr.width, hdr.height, hdr.ncomp = int(size[0]), int(size[1]), len(planes)
    hdr.hs, hdr.vs = (1, 1) if sampling is None else (int(sampling[0]), int(sampling[1]))
    need = _lib_fn("mopa_jpeg_coeff_bytes")(ctypes.addressof(hdr))
    if need == 0:
        raise ValueError(f"{who}: size {tuple(size)}, {len(planes)} components, sampling {sampling} is not a supported image")
    hdr.mcus_x, hdr.mcus_y = -(-hdr.width // (8 * hdr.hs)), -(-hdr.height // (8 * hdr.vs))
    buf = np.zeros(need, np.uint8)
    quant = np.asarray(quant)
    if quant.shape != (hdr.ncomp, 64):
        raise ValueError(f"{who}: quant must be ({hdr.ncomp}, 64), got {quant.shape}")
    buf[:128 * hdr.ncomp] = np.ascontiguousarray(quant, dtype=np.uint16).view(np.uint8).reshape(-1)
    off = 384
    for c, p in enumerate(planes):
        bx, by = hdr.mcus_x * (1 if c else hdr.hs), hdr.mcus_y * (1 if c else hdr.vs)
        p = np.asarray(p)
        if p.shape != (by, bx, 64) or p.dtype != np.int16:
            raise ValueError(f"{who}: plane {c} must be int16 ({by}, {bx}, 64), got {p.dtype} {p.shape}")
        hdr.plane_off[c], hdr.blocks_x[c], hdr.blocks_y[c] = off, bx, by
        hdr.comp_w[c] = hdr.width if c == 0 else -(-hdr.width // hdr.hs)
        hdr.comp_h[c] = hdr.height if c == 0 else -(-hdr.height // hdr.vs)
        for k in range(64):
            hdr.quant[c][k] = int(quant[c, k])
        buf[off:off + p.size * 2] = np.ascontiguousarray(p).view(np.uint8).reshape(-1)
        off += p.size * 2
    hdr.coeff_bytes, hdr.supported = off, 1
    return hdr, torch.from_numpy(buf)


# ------------------------------------------------------------------------------------------------ the device half
def _overlap(a, b):
    """Whether the storage ranges two tensors span overlap."""
    def span(t):
        last = sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
        return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def _check_out(who, out, sizes, device=None):
    """``out``: a list of B uint8 (H, W, 3) tensors on one GPU whose pixels are contiguous (strides (pitch, 3, 1), pitch >= 3 W: a
    wider row pitch is allowed), none overlapping another.  Shapes and dtypes first, then the device."""
    if not isinstance(out, (list, tuple)) or len(out) != len(sizes):
        raise ValueError(f"{who}: out must be a list of {len(sizes)} tensors, one per image")
    for b, (t, (w, h)) in enumerate(zip(out, sizes)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: out[{b}] must be a torch tensor on the GPU, got {type(t).__name__}")
        if t.dtype != torch.uint8:
            raise TypeError(f"{who}: out[{b}] must be uint8, got {t.dtype}")
        if tuple(t.shape) != (h, w, 3):
            raise ValueError(f"{who}: out[{b}] must be ({h}, {w}, 3) for image {b}, got {tuple(t.shape)}")
        if t.stride(2) != 1 or t.stride(1) != 3 or (h > 1 and t.stride(0) < 3 * w):
            raise ValueError(f"{who}: out[{b}] must have strides (pitch >= {3 * w}, 3, 1), got {tuple(t.stride())}")
    for b, t in enumerate(out):
        if not t.is_cuda:
            raise RuntimeError(f"{who}: out[{b}] must be on the GPU (there is no CPU fallback)")
        if t.device != out[0].device or (device is not None and t.device != device):
            raise ValueError(f"{who}: out[{b}] is on {t.device}; all tensors of a call must be on one device")
    for b in range(len(out)):
        for c in range(b):
            if _overlap(out[b], out[c]):
                raise ValueError(f"{who}: out[{b}] overlaps out[{c}]")
    return out[0].device


def decode_coefficients_batch(headers, buffers, out=None, device=None):
    """The device half alone: the headers and coefficient buffers of B images (``decode_entropy`` / ``pack_coefficients``) -> a list
    of B (H, W, 3) uint8 device tensors (``out`` if given, filled in place).  ``buffers``: host tensors (uploaded here, one copy per
    image) or device tensors (16-byte aligned)."""
    who = f"{_NAME}.decode_coefficients_batch"
    headers, buffers = list(headers), list(buffers)
    if not headers or len(headers) != len(buffers):
        raise ValueError(f"{who}: one buffer per header, and at least one")
    for b, (h, t) in enumerate(zip(headers, buffers)):
        if not isinstance(h, Header):
            raise TypeError(f"{who}: headers[{b}] must be a jpegdec.Header, got {type(h).__name__}")
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
            raise TypeError(f"{who}: buffers[{b}] must be a contiguous 1-D uint8 tensor")
    sizes = [(h.width, h.height) for h in headers]
    dev = _check_out(who, out, sizes, device) if out is not None else (torch.device("cuda") if device is None else torch.device(device))
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the device half runs on the GPU (there is no CPU fallback), got device {dev}")
    with torch.cuda.device(dev):
        if out is None:
            out = [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for w, h in sizes]
        bufs = [t if t.is_cuda else t.to(dev, non_blocking=True) for t in buffers]
        for s, e in chunk_ranges(len(headers), _lib.query("mopa_jpeg_max_images")):
            _launch(headers[s:e], [ptr(t) for t in bufs[s:e]], [t.numel() for t in bufs[s:e]], out[s:e])
    return out


def _launch(headers, coeff_ptrs, coeff_bytes, outs):
    B = len(headers)
    harr = (Header * B)(*headers)
    cb = (ctypes.c_int64 * B)(*coeff_bytes)
    pitch = (ctypes.c_int64 * B)(*[t.stride(0) if t.shape[0] > 1 else 3 * t.shape[1] for t in outs])
    cp, dp = host_ptrs(coeff_ptrs), host_ptrs(outs)
    call("mopa_jpeg_decode_batch", host_addr(cp), host_addr(cb), ctypes.addressof(harr), B, host_addr(dp), host_addr(pitch), stream())


class _Staging:
    """One growing pinned buffer: the coefficients of a call.  The asynchronous copies out of it are fenced by an event that the
    next call waits for before it writes into the buffer again."""

    def __init__(self):
        self.buf, self.event = None, None

    def get(self, nbytes):
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = _pinned(max(int(nbytes * 1.25), 1 << 20))
        return self.buf

    def fence(self):
        self.event = torch.cuda.Event()
        self.event.record()


_staging = _Staging()
_pools = {}


def _pool(threads):
    p = _pools.get(threads)
    if p is None:
        p = _pools[threads] = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="mopa-jpeg")
    return p


def decode_jpeg_batch(datas, out=None, threads=None, device=None):
    """B JPEG streams -> a list of B (H, W, 3) uint8 device tensors with Pillow's bits (images of any sizes and samplings in one
    call).  ``datas``: a list of ``bytes`` / ``memoryview`` / 1-D uint8 arrays (host).  ``out``: a list of B uint8 (H, W, 3) device
    tensors to fill instead, pixels contiguous, rows at any pitch >= 3 W (views of a wider buffer); one that overlaps another, or has
    the wrong shape, dtype or device, is refused.  ``threads``: the size of the entropy stage's pool (default 4; 1 = the calling
    thread).

    The markers of every stream are read first, then the entropy stage of all images runs (on the pool) into one pinned buffer:
    ``JpegUnsupported`` (decode that file with Pillow) and ``JpegDataError`` are raised before anything is launched.  Then, per chunk
    of up to 32 images: one asynchronous copy of the chunk's coefficients, one launch.  No read-back."""
    who = f"{_NAME}.decode_jpeg_batch"
    if isinstance(datas, (bytes, bytearray, memoryview, np.ndarray, torch.Tensor)):
        raise TypeError(f"{who}: datas must be a list of streams, got one {type(datas).__name__}")
    views = [_bytes_view(d, who, f"datas[{b}]") for b, d in enumerate(datas)]
    if not views:
        raise ValueError(f"{who}: no streams")
    threads = DEFAULT_THREADS if threads is None else int(threads)
    if threads < 1 or threads > 64:
        raise ValueError(f"{who}: threads must be in 1..64, got {threads}")
    headers = []
    for b, v in enumerate(views):
        rc, h = _info(v, who, f"datas[{b}]: ")
        _raise_for(rc, h, who, f"datas[{b}]: ")
        headers.append(h)
    sizes = [(h.width, h.height) for h in headers]
    dev = _check_out(who, out, sizes, None if device is None else torch.device(device)) if out is not None else \
        (torch.device("cuda") if device is None else torch.device(device))
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the device half runs on the GPU (there is no CPU fallback), got device {dev}")
    offs, total = [], 0
    for h in headers:
        offs.append(total)
        total += -(-int(h.coeff_bytes) // _ALIGN) * _ALIGN
    with torch.cuda.device(dev):
        stage = _staging.get(total)
        base = stage.data_ptr()
        fn = _lib_fn("mopa_jpeg_entropy_decode")

        def entropy(b):
            return fn(views[b].ctypes.data, ctypes.addressof(headers[b]), base + offs[b], views[b].size, int(headers[b].coeff_bytes))

        rcs = [entropy(b) for b in range(len(views))] if threads == 1 or len(views) == 1 else list(_pool(threads).map(entropy, range(len(views))))
        for b, rc in enumerate(rcs):
            _raise_for(rc, headers[b], who, f"datas[{b}]: ")
        if out is None:
            out = [torch.empty((h, w, 3), dtype=torch.uint8, device=dev) for w, h in sizes]
        for s, e in chunk_ranges(len(views), _lib.query("mopa_jpeg_max_images")):
            lo, hi = offs[s], (offs[e] if e < len(views) else total)
            devbuf = torch.empty(hi - lo, dtype=torch.uint8, device=dev)
            devbuf.copy_(stage[lo:hi], non_blocking=True)
            _launch(headers[s:e], [devbuf.data_ptr() + offs[b] - lo for b in range(s, e)],
                    [int(headers[b].coeff_bytes) for b in range(s, e)], out[s:e])
        _staging.fence()
    return list(out)
