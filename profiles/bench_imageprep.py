#!/usr/bin/env python3
"""prepare_batch (mopa_amd/imageprep.py, csrc/imageprep.hip) at the 8 + 8 nuScenes batch and the 8 + 8 SemanticKITTI batch: HIP-event
time around one call (host enqueue included), median of 50 after 5 warm-up calls; launch count from the library's own call log;
achieved share of HBM bandwidth on the algorithmic bytes (raw image + mask + points in, img + ori_img + mask + indices out) against
6.3 TB/s achievable.  Where Pillow and scipy are installed the host path of the same batch is timed too (one thread, the calls
the datasets make per sample; refine_sam_mask restated with torch.unique + one compare per id); otherwise that row is left out.
``--hue`` puts a hue step (operation 3, between the first and the second blend) into every sample's jitter.
Writes a markdown table to stdout (and to the file named on the command line, if one is)."""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from mopa_amd import _lib, imageprep as ip  # noqa: E402

HBM = 6.3e12
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
SHAPES = [("nuScenes 8 + 8, 1600x900 -> 400x225", 1600, 900, (400, 225), None, 3500),
          ("SemanticKITTI 8 + 8, 1242x375, crop 480x302", 1242, 375, None, (480, 302), 12000)]
ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def make(W, H, crop, n, B=16, seed=0, hue=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for b in range(B):
        coarse = rng.integers(0, 256, (H // 8 + 1, W // 8 + 1, 3))
        img = np.clip(np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:H, :W] + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)
        mask = np.repeat(np.repeat(rng.integers(0, 120, (H // 32 + 1, W // 32 + 1)), 32, 0), 32, 1)[:H, :W].astype(np.uint8)
        pts = np.stack([rng.random(n) * (H * 0.6 - 1) + H * 0.4, rng.random(n) * (W - 1)], 1).astype(np.float32)
        s = {"image": img, "sam_mask": mask, "points_img": pts, "jitter": (ORDERS[b % 6], (0.8 + 0.03 * b, 1.3 - 0.02 * b, 1.1)),
             "flip": b % 2 == 1}
        if hue:
            order, fs = s["jitter"]
            s["jitter"] = (order[:1] + (3,) + order[1:], fs[:1] + (0.1 - 0.0125 * b,) + fs[1:])
        if crop:
            left = int(rng.random() * (W + 1 - crop[0]))
            s["crop"] = (left, H - crop[1], left + crop[0], H)
        out.append(s)
    return out


def host_path(samples, resize):
    """The datasets' per-sample calls on one thread."""
    from PIL import Image, ImageEnhance
    from scipy.ndimage import zoom
    for s in samples:
        im = Image.fromarray(s["image"])
        p = s["points_img"].copy()
        mask = s["sam_mask"]
        if resize:
            p[:, 0] = float(resize[1]) / im.size[1] * np.floor(p[:, 0])
            p[:, 1] = float(resize[0]) / im.size[0] * np.floor(p[:, 1])
            im = im.resize(resize, Image.BILINEAR)
            mask = zoom(mask, (0.25, 0.25), order=0)
        m = torch.from_numpy(np.ascontiguousarray(mask)).int()
        ids, cnt = torch.unique(m, return_counts=True)
        for i in torch.unique(ids[torch.argsort(cnt, descending=True)]):
            sel = m == i
            if torch.sum(sel) >= 0.1 * (m.shape[0] * m.shape[1]):
                m[sel] = -100
        m[:int(np.min(p, axis=0)[0])] = -100
        if "crop" in s:
            l, t, r, b = s["crop"]
            im = im.crop((l, t, r, b))
            m = m[t:b, l:r]
        for op, f in zip(*s["jitter"]):
            if op == 3:                                           # torchvision's adjust_hue on a PIL image
                hh, ss, vv = im.convert("HSV").split()
                np_h = np.array(hh, dtype=np.uint8)
                with np.errstate(over="ignore"):
                    np_h += np.int32(f * 255).astype(np.uint8)
                im = Image.merge("HSV", (Image.fromarray(np_h, "L"), ss, vv)).convert("RGB")
                continue
            im = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](im).enhance(f)
        x = np.array(im, dtype=np.float32) / 255.
        if s["flip"]:
            x = np.ascontiguousarray(np.fliplr(x))
        x = (x - np.asarray(NORM[0], np.float32)) / np.asarray(NORM[1], np.float32)
        np.moveaxis(x, -1, 0)
        p.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="also write the table to this file")
    ap.add_argument("--hue", action="store_true", help="a hue step in every sample's jitter")
    args = ap.parse_args()
    lines = ["| batch | path | µs (median) | launches | algorithmic MB | GB/s | of 6.3 TB/s |", "|---|---|---|---|---|---|---|"]
    for name, W, H, resize, crop, n in SHAPES:
        host = make(W, H, crop, n, hue=args.hue)
        samples = [{k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in host]
        w, h = resize or crop
        out = torch.empty(16, 3, h, w, device="cuda")

        def run():
            return ip.prepare_batch(samples, out=out, resize=resize, normalizer=NORM, ema_input=True)
        names = []
        orig = _lib.call
        ip.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
        run()
        ip.call = orig
        # kernels behind the entry points: the mask call is two, the others one; memsets (sums, counts, row minima) not counted
        kernels = sum(2 if nm == "mopa_imageprep_mask" else 1 for nm in names)
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(50):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        us = statistics.median(ts)
        oh, ow = (H, W) if crop else (h, w)                       # ori_img: the uncropped image for SemanticKITTI
        byts = 16 * (H * W * 3 + H * W + n * 8 + h * w * 12 + oh * ow * 12 + h * w * 4 + 2 * n * 16)
        lines.append(f"| {name} | prepare_batch{' with hue' if args.hue else ''} | {us:,.1f} | {kernels} | {byts / 1e6:.1f} | {byts / us / 1e3:,.0f} | {byts / (us * 1e-6) / HBM:.3f} |")
        try:
            import PIL  # noqa: F401
            import scipy  # noqa: F401
        except ImportError:
            continue
        torch.set_num_threads(1)
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_path(host, resize)
            hs.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"| {name} | host path (Pillow, scipy; one thread) | {statistics.median(hs):,.1f} | | | | |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
