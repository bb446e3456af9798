"""Encoded camera images of either kind -> ``(H, W, 3)`` uint8 device tensors with Pillow's bits: JPEG streams go through
``jpegdec.decode_jpeg_batch``, PNG streams through ``pngdec.decode_png_batch``, told apart by their signatures."""
from __future__ import annotations

import io

import numpy as np
import torch

from . import jpegdec, pngdec
from .jpegdec import JpegDataError, JpegUnsupported, _bytes_view  # noqa: F401  (the exceptions a caller catches)
from .pngdec import PngDataError, PngUnsupported  # noqa: F401

_NAME = "imagedec"


def _pillow():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def sniff(data) -> str:
    """"jpeg" / "png" by the stream's first bytes; anything else is a ``ValueError``."""
    head = bytes(memoryview(data)[:8])
    if head == pngdec.SIGNATURE:
        return "png"
    if head[:2] == b"\xff\xd8":
        return "jpeg"
    raise ValueError(f"{_NAME}: neither a JPEG nor a PNG stream (it starts with {head!r})")


def decode_images(datas, threads=None, device=None, fallback=True):
    """A list of JPEG and PNG streams (host bytes) -> a list of (H, W, 3) uint8 device tensors in input order: what
    ``np.asarray(Image.open(...).convert("RGB"))`` returns for each.  All JPEGs of the call go through one ``decode_jpeg_batch``,
    all PNGs through one ``decode_png_batch`` (``threads``: their host pools).

    ``fallback``: a stream outside a decoder's supported subset (``jpeg_info`` / ``png_info`` say so: progressive JPEG, 16-bit or
    interlaced PNG, ...) is decoded by Pillow on the host and uploaded, if Pillow can be imported; with ``fallback=False``, or without
    Pillow, ``JpegUnsupported`` / ``PngUnsupported`` propagates.  ``JpegDataError`` / ``PngDataError`` always propagate."""
    who = f"{_NAME}.decode_images"
    if isinstance(datas, (bytes, bytearray, memoryview, np.ndarray, torch.Tensor)):
        raise TypeError(f"{who}: datas must be a list of streams, got one {type(datas).__name__}")
    views = [_bytes_view(d, who, f"datas[{b}]") for b, d in enumerate(datas)]
    if not views:
        raise ValueError(f"{who}: no streams")
    dev = torch.device("cuda") if device is None else torch.device(device)
    Image = _pillow() if fallback else None
    lists = {"jpeg": [], "png": [], "pillow": []}
    for b, v in enumerate(views):
        kind = sniff(v)
        if Image is not None and not (jpegdec.jpeg_info(v) if kind == "jpeg" else pngdec.png_info(v)).supported:
            kind = "pillow"
        lists[kind].append(b)
    out = [None] * len(views)
    for kind, fn in (("jpeg", jpegdec.decode_jpeg_batch), ("png", pngdec.decode_png_batch)):
        if lists[kind]:
            for b, t in zip(lists[kind], fn([views[b] for b in lists[kind]], threads=threads, device=dev)):
                out[b] = t
    for b in lists["pillow"]:
        arr = np.array(Image.open(io.BytesIO(views[b].tobytes())).convert("RGB"))
        out[b] = torch.from_numpy(arr).to(dev)
    return out
