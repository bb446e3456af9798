#!/usr/bin/env python3
"""mopa_amd/jpegdec.py (csrc/jpeg_entropy.h + csrc/jpegdec.hip) at 1 and 16 images of the full-size shape (the 1600 x 900 4:2:0
quality-75 stream of tests/golden/g16_jpegdec.npz), median of 50 after 5 warm-up calls, the spread (min - max) beside each median.

Host, one thread, wall clock per image:
  entropy stage alone      mopa_jpeg_entropy_decode into a pageable and into a pinned buffer
  decode_jpeg_batch        the whole Python call, threads=1 (and with the default pool), until the device has finished
  Pillow                   np.asarray(Image.open(...).convert("RGB")) on this machine, if Pillow can be imported (else said so),
                           and that call plus the upload of the decoded array
Device, HIP events:
  upload                   the chunk's coefficients from the pinned buffer (one copy)
  device half              the launch over resident coefficients (decode_coefficients_batch), with the share of the achievable HBM rate
                           (6.3 TB/s) its floor traffic reaches: coefficient planes read once, RGB written once
Kernel times come from a profiler run of `--device-only` (which only loops the device half), see profiles/r27_jpegdec.md.
Writes a markdown table to stdout (and to the file named after --out)."""
import argparse
import ctypes
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from mopa_amd import jpegdec as jd  # noqa: E402

HBM = 6.3e12          # achievable bytes / s
FIXTURE = os.path.join("tests", "golden", "g16_jpegdec.npz")


def events(fn, warm=5, n=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def wall(fn, warm=5, n=50):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts), min(ts), max(ts)


def row(lines, B, what, t, per_image=True, extra=""):
    med, lo, hi = t
    k = B if per_image else 1
    lines.append(f"| {B} | {what} | {med / k:,.1f} | {lo / k:,.1f} – {hi / k:,.1f} | {extra} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--device-only", action="store_true", help="loop the device half of 16 images 50 times and exit (for a profiler run)")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    torch.set_num_threads(1)
    data = np.load(FIXTURE)["full_jpg"].tobytes()
    hdr, coeff = jd.decode_entropy(data)
    W, H = hdr.width, hdr.height
    planes = sum(hdr.blocks_x[c] * hdr.blocks_y[c] * 64 for c in range(hdr.ncomp))
    floor = planes * 2 + W * H * 3          # int16 coefficients, RGB
    lib = jd._lib.load()
    lines = [f"{args.tag}", "", "| images | what | µs per image (median) | min – max | note |", "|---|---|---|---|---|"]

    if args.device_only:
        B = 16
        bufs, outs = [coeff.cuda() for _ in range(B)], [torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
        for _ in range(55):
            jd.decode_coefficients_batch([hdr] * B, bufs, out=outs)
        torch.cuda.synchronize()
        print("device-only loop done")
        return

    # ---- host
    arr = np.frombuffer(data, np.uint8)
    h2 = jd.Header()
    pageable = np.zeros(hdr.coeff_bytes, np.uint8)
    pinned = torch.empty(hdr.coeff_bytes, dtype=torch.uint8, pin_memory=True)
    for name, addr in (("pageable", pageable.ctypes.data), ("pinned", pinned.data_ptr())):
        t = wall(lambda: lib.mopa_jpeg_entropy_decode(arr.ctypes.data, ctypes.addressof(h2), addr, arr.size, hdr.coeff_bytes))
        row(lines, 1, f"entropy stage alone, into a {name} buffer (host, one thread)", t, extra=f"{len(data):,} B in, {hdr.coeff_bytes:,} B out")
    assert np.array_equal(pageable, coeff.numpy()) and torch.equal(pinned, coeff)
    try:
        from PIL import Image
    except ImportError:
        Image = None
        lines.append("| 1 | Pillow | not importable on this machine | | |")
    if Image is not None:
        row(lines, 1, "Pillow: np.asarray(Image.open(...).convert('RGB')) (host, one thread)", wall(lambda: np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))))

        def pil_upload():
            t = torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))).cuda()
            torch.cuda.synchronize()
            return t
        row(lines, 1, "Pillow + upload of the decoded array, synchronised", wall(pil_upload))
        assert torch.equal(pil_upload(), jd.decode_jpeg_batch([data])[0]), "the device path differs from this machine's Pillow"

    for B in (1, 16):
        datas = [data] * B
        outs = [torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]

        def whole(threads):
            jd.decode_jpeg_batch(datas, out=outs, threads=threads)
            torch.cuda.synchronize()

        row(lines, B, "decode_jpeg_batch, threads=1, synchronised (host wall clock)", wall(lambda: whole(1)))
        if B > 1:
            row(lines, B, f"decode_jpeg_batch, threads={jd.DEFAULT_THREADS} (default), synchronised (host wall clock)", wall(lambda: whole(None)))
        torch.cuda.synchronize()
        # ---- device
        stage = torch.empty(B * hdr.coeff_bytes, dtype=torch.uint8, pin_memory=True)
        dev = torch.empty(B * hdr.coeff_bytes, dtype=torch.uint8, device="cuda")
        t = events(lambda: dev.copy_(stage, non_blocking=True))
        row(lines, B, "upload of the coefficients, one copy from pinned memory (HIP events)", t,
            extra=f"{B * hdr.coeff_bytes / (t[0] * 1e-6) / 1e9:.1f} GB/s")
        bufs = [coeff.cuda() for _ in range(B)]
        t = events(lambda: jd.decode_coefficients_batch([hdr] * B, bufs, out=outs))
        row(lines, B, "device half, one launch (HIP events around the Python call)", t,
            extra=f"{B * floor / (t[0] * 1e-6) / HBM:.3f} of 6.3 TB/s on {floor / 1e6:.2f} MB floor traffic per image")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
