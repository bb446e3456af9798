#!/usr/bin/env python3
"""mopa_amd/a2d2prep.py (csrc/a2d2prep.hip) at 1 and 8 frames of 1920 x 1208 with 12,000 lidar points each, the camera's map
prebuilt: HIP-event time around the whole Python call with resident inputs (host argument checks included), median of 50 after 5
warm-up calls, for
  undistort_map            the map build alone (once per camera)
  undistort_images         the remap of the B images alone, with the share of the
                           achievable HBM bandwidth (6.3 TB/s) its floor traffic reaches: per plane 6.96 MB read + 6.96 MB written,
                           plus 13.9 MB of map (9.3 MB xy + 4.6 MB frac) per call
  prepare_frames_a2d2      images + points (two launches), and with the label planes as well
Beside it the same work in numpy on the host of the GPU machine, one thread: the restatement tests/_a2d2_reference.py (remap of the
image and of the label image, labels, casts; median of 3 for one frame, one run for eight).  cv2 itself is NOT installed, so
cv2.undistort was not timed.  Writes a markdown table to stdout (and to argv[1] if given)."""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import _a2d2_reference as ref  # noqa: E402
from mopa_amd import a2d2prep as ap  # noqa: E402

HBM = 6.3e12          # achievable bytes / s
N_POINTS = 12000


def make(B, W, H, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        pts, row, col, refl = ref.lidar_points(rng, N_POINTS, W, H)
        out.append({"image": rng.integers(0, 256, (H, W, 3)).astype(np.uint8), "label_image": ref.block_labels(W, H), "points": pts,
                    "row": row, "col": col, "reflectance": refl})
    return out


def timed(fn, warm=5, n=50):
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


def host_path(samples, xy, frac):
    for s in samples:
        ref.remap(s["image"], xy, frac)
        und = ref.remap(s["label_image"], xy, frac)
        ref.prepare_frame(und, s["points"], s["row"], s["col"], s["reflectance"], ref.TABLE)


def main():
    torch.set_num_threads(1)
    W, H, cam = ref.FULL
    lines = ["| frames | path | µs (median) | min – max | C-ABI calls | share of 6.3 TB/s |", "|---|---|---|---|---|---|"]
    med, lo, hi = timed(lambda: ap.undistort_map(cam, (W, H)))
    lines.append(f"| – | undistort_map, {W} x {H} (once per camera) | {med:,.1f} | {lo:,.1f} – {hi:,.1f} | 1 | |")
    umap = ap.undistort_map(cam, (W, H))
    xy, frac = umap.xy.cpu().numpy(), umap.frac.cpu().numpy()
    table = torch.from_numpy(ref.TABLE).cuda()
    plane, mapb = W * H * 3, W * H * 6
    for B in (1, 8):
        host = make(B, W, H)
        dev = [{k: torch.from_numpy(v).cuda() for k, v in s.items()} for s in host]
        imgs = torch.stack([s["image"] for s in dev])
        out = torch.empty_like(imgs)
        med, lo, hi = timed(lambda: ap.undistort_images(imgs, umap, out=out))
        share = (2 * plane * B + mapb) / (med * 1e-6) / HBM
        lines.append(f"| {B} | undistort_images | {med:,.1f} | {lo:,.1f} – {hi:,.1f} | 1 | {share:.2f} |")
        for with_label in (False, True):
            names = []
            orig = ap.call
            ap.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
            res = ap.prepare_frames_a2d2(dev, umap, table, with_label_image=with_label)
            ap.call = orig
            assert int(res["bad_index"].sum()) == 0
            med, lo, hi = timed(lambda: ap.prepare_frames_a2d2(dev, umap, table, with_label_image=with_label))
            what = "images, label planes and points" if with_label else "images and points"
            lines.append(f"| {B} x {N_POINTS:,} points | prepare_frames_a2d2, {what} | {med:,.1f} | {lo:,.1f} – {hi:,.1f} | {len(names)} | |")
        hs = []
        for _ in range(3 if B == 1 else 1):
            t0 = time.perf_counter()
            host_path(host, xy, frac)
            hs.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"| {B} x {N_POINTS:,} points | numpy restatement on the host, one thread (cv2 absent) | {statistics.median(hs):,.0f} | {min(hs):,.0f} – {max(hs):,.0f} | | |")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
