#!/usr/bin/env python3
"""prepare_scans_nuscenes (mopa_amd/nuscprep.py, csrc/nuscprep.hip) at 1 and 8 sweeps of 34,720 points (32 beams x 1,085), image
1600 x 900, 40 boxes per sweep, ground index lists of a third of the points: HIP-event time around one call with resident scans
(host argument checks, the upload of the calibration and boxes, the host-side proj_matrix and the one read-back included),
median of 50 after 5 warm-up calls; C-ABI calls per call (the same for 1 and 8 sweeps: every kernel covers all scans); and the two
host-only parts of the call timed alone (wall clock, median of 200): the argument checks and the numpy proj_matrix.

Beside it the same work in numpy on the host of the GPU machine, one thread, median of 3: map_pointcloud_to_image's expressions
plus the box loop of preprocess.py (tests/_nuscenes_reference.py::preprocess_scan_numpy; pyquaternion and nuscenes-devkit are
absent, their functions are restated from the published definitions).  Writes a markdown table to stdout (and to argv[1] if given)."""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import _nuscenes_reference as ref  # noqa: E402
from mopa_amd import _lib, nuscprep as npr  # noqa: E402


def make(B, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = ref.FULL["beams"] * ref.FULL["per_beam"]
    out = []
    for _ in range(B):
        calib = ref.nusc_calib(rng)
        boxes, cls = ref.view_boxes(rng, calib, ref.FULL["boxes"])
        out.append({"scan": ref.lidar_sweep(rng, n, boxes), "calib": calib, "boxes": boxes, "box_class": cls,
                    "g": np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)})
    return out


def host_path(samples):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return [len(ref.preprocess_scan_numpy(s["scan"], s["calib"], s["boxes"], s["box_class"], ref.NUSC_SIZE, g=s["g"])["points"]) for s in samples]


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


def main():
    lines = ["| sweeps | path | µs (median) | min – max | C-ABI calls | kept points |", "|---|---|---|---|---|---|"]
    torch.set_num_threads(1)
    for B in (1, 8):
        host = make(B)
        dev = [{"scan": torch.from_numpy(s["scan"]).cuda(), "calib": s["calib"], "boxes": s["boxes"], "box_class": s["box_class"],
                "g_indices": torch.from_numpy(s["g"]).cuda()} for s in host]

        def run():
            return npr.prepare_scans_nuscenes(dev, ref.NUSC_SIZE)
        names = []
        orig = _lib.call
        npr.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
        res = run()
        npr.call = orig
        want = host_path(host)
        assert res["counts"].tolist() == want, "the device and the numpy flow disagree on the counts"
        med, lo, hi = timed(run)
        lines.append(f"| {B} x 34,720 | prepare_scans_nuscenes, 40 boxes, ground lists | {med:,.1f} | {lo:,.1f} – {hi:,.1f} | {len(names)} | {sum(want):,} |")
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_path(host)
            hs.append((time.perf_counter() - t0) * 1e6)
        # the host side of the call alone, wall clock, median of 200: what does not shrink with a faster device
        for what, fn in (("argument checks (`_check`)", lambda: npr._check(dev, ref.NUSC_SIZE, None)),
                         ("numpy `proj_matrix` of every sample", lambda: [npr.proj_matrix(s["calib"]) for s in dev])):
            ws = []
            for _ in range(200):
                t0 = time.perf_counter()
                fn()
                ws.append((time.perf_counter() - t0) * 1e6)
            lines.append(f"| {B} x 34,720 | host part of the call: {what} | {statistics.median(ws):,.1f} | {min(ws):,.1f} – {max(ws):,.1f} | | |")
        lines.append(f"| {B} x 34,720 | numpy on the host, one thread | {statistics.median(hs):,.1f} | {min(hs):,.1f} – {max(hs):,.1f} | | {sum(want):,} |")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
