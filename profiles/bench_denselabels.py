#!/usr/bin/env python3
"""prepare_dense_pslabels (mopa_amd/imageprep.py, csrc/denselabels.hip) at the SemanticKITTI shape -- 370 x 1226 masks with about
200 ids, 20,000 points per sample -- for B = 1 and B = 8, uncropped and with the 480 x 302 bottom crop + flip: HIP-event time around
one Python call (host enqueue included), median and quartiles of 50 after 5 warm-up calls; entry-point calls from the library's own
call log (the kernels behind one call are fixed: 13 and two memsets).  Beside them the host path the
datasets run per sample, restated with torch on ONE thread (the (H, W, C) float tensor, per-class median, index_put, and per mask id
a full-image compare, a gather, a sum and a masked store), and prepare_batch of the 8-sample cropped batch with and without the
pseudo-label keys, as alternating calls, so that the cost of the added stage is read against the spread.
Writes a markdown table to stdout (and to the file named on the command line, if one is)."""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from mopa_amd import _lib, imageprep as ip  # noqa: E402

H, W, N, IDS, C = 370, 1226, 20000, 240, 10       # 240 draws over 468 blocks: about 200 distinct ids
CROP = (480, 302)
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def make(B, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for b in range(B):
        mask = np.repeat(np.repeat(rng.integers(1, IDS, (H // 32 + 1, W // 32 + 1)), 32, 0), 32, 1)[:H, :W].astype(np.uint8)
        mask[:H * 3 // 10] = 0                                    # one id above the area threshold, where no lidar point falls
        pts = np.stack([rng.random(N) * (H * 0.7 - 1) + H * 0.3, rng.random(N) * (W - 1)], 1).astype(np.float32)
        at = mask[pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)].astype(np.int64)
        labels = np.where(rng.random(N) < 0.75, (at * 7 + 3) % C, rng.integers(0, C, N)).astype(np.uint8)
        probs = (0.35 + 0.65 * rng.random(N)).astype(np.float32)
        left = int(rng.random() * (W + 1 - CROP[0]))
        img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        out.append({"image": img, "sam_mask": mask, "points_img": pts, "probs_2d": probs, "pseudo_label_2d": labels,
                    "crop": (left, H - CROP[1], left + CROP[0], H), "flip": b % 2 == 1})
    return out


def host_path(s, crop):
    """What the dataset does for one sample, on the host."""
    p, raw = s["probs_2d"], s["pseudo_label_2d"].astype(np.int64)
    rows = np.zeros((len(p), C))
    rows += ((1 - p) / (C - 1))[:, None]
    rows[np.arange(len(p)), raw] = p
    probs = torch.from_numpy(rows).float()
    idx = torch.from_numpy(s["points_img"]).int().long()
    mask = torch.from_numpy(s["sam_mask"])
    conf, lab = probs.max(1)[0], probs.argmax(1)
    refined = lab.clone()
    for c in lab.unique():
        sel = torch.nonzero(lab == c).squeeze(1)
        thresh = min(conf[sel].median(), 0.9)
        refined[sel[conf[sel] < thresh]] = -100
    probs[refined <= -100] = 0.0
    dense = torch.full(mask.shape, -100, dtype=torch.int32)
    full = torch.zeros(mask.shape[0], mask.shape[1], C)
    dense[idx[:, 0], idx[:, 1]] = refined.int()
    full[idx[:, 0], idx[:, 1]] = probs
    for i in torch.unique(mask):
        sel = mask == i
        if torch.sum(sel) >= 0.1 * (mask.shape[0] * mask.shape[1]):
            continue
        dense[sel] = full[sel].sum(0).argmax(0).int()
    out = dense.numpy()
    if crop:
        l, t, r, b = s["crop"]
        out = out[t:b, l:r]
        if s["flip"]:
            out = np.ascontiguousarray(np.fliplr(out))
    return out


def timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return ts


def quart(ts):
    q = statistics.quantiles(ts, n=4)
    return f"{statistics.median(ts):,.1f} | {q[0]:,.1f} .. {q[2]:,.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", help="also write the table to this file")
    ap.add_argument("--no-host", action="store_true", help="leave out the host path")
    args = ap.parse_args()
    lines = ["| what | B | µs per call (median) | quartiles | entry-point calls | µs per sample |", "|---|---|---|---|---|---|"]
    host = make(8)
    dev = [{k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in host]
    checked = False
    for B in (1, 8):
        ss = dev[:B]
        arrays = [[s[k] for s in ss] for k in ("probs_2d", "pseudo_label_2d", "points_img", "sam_mask")]
        for crop in (False, True):
            kw = dict(windows=[s["crop"] for s in ss], flip=[s["flip"] for s in ss]) if crop else {}
            out = torch.empty(B, *(CROP[::-1] if crop else (H, W)), dtype=torch.int32, device="cuda")

            def run():
                return ip.prepare_dense_pslabels(*arrays, num_classes=C, out=out, **kw)
            names = []
            orig = _lib.call
            ip.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
            run()
            ip.call = orig
            ts = timed(run)
            what = "prepare_dense_pslabels, " + ("480 x 302 bottom crop + flip" if crop else "370 x 1226 uncropped")
            lines.append(f"| {what} | {B} | {quart(ts)} | {len(names)} | {statistics.median(ts) / B:,.1f} |")
            if not checked and not args.no_host:                   # the two paths compute one thing (every id of this input is decided)
                torch.set_num_threads(1)
                assert np.array_equal(out[0].cpu().numpy(), host_path(host[0], crop)), "device and host path differ"
                checked = True
    if not args.no_host:
        torch.set_num_threads(1)
        for crop in (False, True):
            hs = []
            for s in host[:4]:
                t0 = time.perf_counter()
                host_path(s, crop)
                hs.append((time.perf_counter() - t0) * 1e6)
            lines.append(f"| host path, one thread, {'cropped' if crop else 'uncropped'} | 1 | {statistics.median(hs):,.1f} | "
                         f"{min(hs):,.1f} .. {max(hs):,.1f} (of 4) | | {statistics.median(hs):,.1f} |")
    # prepare_batch of the cropped 8-sample batch with and without the keys, alternating
    with_keys = dev
    without = [{k: v for k, v in s.items() if k not in ("probs_2d", "pseudo_label_2d")} for s in dev]
    img = torch.empty(8, 3, CROP[1], CROP[0], device="cuda")
    t_with, t_without = [], []
    for samples in (with_keys, without):
        for _ in range(5):
            ip.prepare_batch(samples, out=img, normalizer=NORM)
    for _ in range(50):
        t_without += timed(lambda: ip.prepare_batch(without, out=img, normalizer=NORM), reps=1, warm=0)
        t_with += timed(lambda: ip.prepare_batch(with_keys, out=img, normalizer=NORM), reps=1, warm=0)
    lines.append(f"| prepare_batch without the keys (alternating) | 8 | {quart(t_without)} | | {statistics.median(t_without) / 8:,.1f} |")
    lines.append(f"| prepare_batch with probs_2d / pseudo_label_2d (alternating) | 8 | {quart(t_with)} | | {statistics.median(t_with) / 8:,.1f} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
