#!/usr/bin/env python3
"""mopa_amd/pngdec.py (host inflate + csrc/pngdec.hip) at 1, 8 and 16 images of the two camera shapes (376 x 1241 and 1208 x 1920
RGB: the seeded synthetic image of tests/_png_reference.py::synthetic_rgb, all five filters cycling over the rows, zlib level 6),
median of 50 after 5 warm-up calls, the spread (min - max) beside each median.

Host, wall clock per image:
  Pillow                   np.asarray(Image.open(...).convert("RGB")) on this machine, one thread, if Pillow can be imported (else said so)
  host half alone          chunk walk + inflate + the copy into the pinned staging buffer (what decode_png_batch does before the copy)
  decode_png_batch         the whole Python call at threads = 1 and 4, until the device has finished
Device, HIP events around the Python call:
  device half              the launch over resident scanlines (decode_scanlines_batch), with the share of the achievable HBM rate
                           (6.3 TB/s) its floor traffic reaches: scanlines read once, RGB written once
Writes a markdown table to stdout (and to the file named after --out)."""
import argparse
import io
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import _png_reference as ref  # noqa: E402
from mopa_amd import pngdec as pd  # noqa: E402

HBM = 6.3e12          # achievable bytes / s


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


def row(lines, shape, B, what, t, extra=""):
    med, lo, hi = t
    lines.append(f"| {shape} | {B} | {what} | {med / B:,.0f} | {lo / B:,.0f} – {hi / B:,.0f} | {extra} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--tag", default="")
    ap.add_argument("--n", type=int, default=50)
    args = ap.parse_args()
    torch.set_num_threads(1)
    lines = [args.tag, "", "| shape | images | what | µs per image (median) | min – max | note |", "|---|---|---|---|---|---|"]
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for H, W in ((376, 1241), (1208, 1920)):
        shape = f"{H} x {W}"
        img = ref.synthetic_rgb(H, W, 18)
        data = ref.encode_png(img, 2, np.arange(H) % 5, level=6)
        hdr, scan = pd.inflate_scanlines(data)
        floor = hdr.scan_bytes + H * W * 3
        note = f"{len(data):,} B in ({len(data) / (H * W * 3):.2f} of raw), {hdr.scan_bytes:,} B of scanlines"
        if Image is None:
            lines.append(f"| {shape} | 1 | Pillow | not importable on this machine | | |")
        else:
            row(lines, shape, 1, "Pillow: np.asarray(Image.open(...).convert('RGB')) (host, one thread)",
                wall(lambda: np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), n=args.n), note)
            assert np.array_equal(pd.decode_png_batch([data])[0].cpu().numpy(), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
        stage = torch.empty(hdr.scan_bytes, dtype=torch.uint8, pin_memory=True)
        row(lines, shape, 1, "host half alone: chunk walk, inflate, copy into a pinned buffer (one thread)",
            wall(lambda: pd.inflate_scanlines(data, out=stage), n=args.n))
        for B in (1, 8, 16):
            datas = [data] * B
            outs = [torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]

            def whole(threads):
                pd.decode_png_batch(datas, out=outs, threads=threads)
                torch.cuda.synchronize()

            for threads in (1, 4) if B > 1 else (1,):
                row(lines, shape, B, f"decode_png_batch, threads={threads}, synchronised (host wall clock)", wall(lambda: whole(threads), n=args.n))
            assert all(np.array_equal(o.cpu().numpy(), img) for o in outs[:2])
            bufs = [scan.cuda() for _ in range(B)]
            t = events(lambda: pd.decode_scanlines_batch([hdr] * B, bufs, out=outs), n=args.n)
            row(lines, shape, B, "device half, one launch (HIP events around the Python call)", t,
                f"{B * floor / (t[0] * 1e-6) / HBM:.4f} of 6.3 TB/s on {floor / 1e6:.2f} MB floor traffic per image")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
