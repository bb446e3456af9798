#!/usr/bin/env python3
"""estimate_ground_batch (mopa_amd/ground.py, csrc/ground.hip) for 8 scans of the nuScenes shape (34,880 points each) and 8 of the
SemanticKITTI shape (120,000 points each), synthetic sweeps of mopa_amd/synth.py, seeds 0-7, resident on the device: HIP-event time
around one call (the host's enqueue, torch.cat of the list and the upload of the 2 (B + 1)-entry table included; nothing is read
back), median of 50 after 5 warm-up calls, with min and max as the spread.  Each shape is measured in a child process of its own
under a time limit, so that a hang in one ends that measurement only.

Beside it: the kernel launches of one call for batch 1 and batch 8 (mopa_ground_launches: they must be equal) and the C-ABI calls,
and the float64 numpy restatement (tests/_ground_reference.py) over the same 8 scans on one host thread, median of 3 -- the host
figure, on the CPU of the machine that holds the GPU.  The device masks are held against the restatement's before anything is
timed.  Writes a markdown table to stdout (and to argv[1] if given).  There is no earlier device path to compare with: the time is
reported, not gated."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIMIT = 240     # seconds per shape
B = 8


def one(shape_name):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ground_reference as ref
    from mopa_amd import _lib, ground, synth
    torch.set_num_threads(1)
    shape = getattr(synth, shape_name)
    h = shape["height"]
    prm = ground.GroundParams(sensor_height=h)
    host = [synth.lidar_points(seed, shape) for seed in range(B)]
    dev = [torch.from_numpy(p).cuda() for p in host]
    rows = _lib.query("mopa_ground_rows_per_block")

    def launches(sets):
        return _lib.query("mopa_ground_launches", sum(-(-len(p) // rows) for p in sets))
    names = []
    orig = _lib.call
    ground.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
    got = ground.estimate_ground_batch(dev, prm)
    ground.call = orig
    # the same answer as the restatement before anything is timed
    hs, n_ground, n_fragile = [], 0, 0
    for rep in range(3):
        t0 = time.perf_counter()
        want = [ref.estimate(p, h) for p in host]
        hs.append((time.perf_counter() - t0) * 1e3)
    for g, (mask, fragile) in zip(got, want):
        assert int(((g.cpu().numpy() != mask) & ~fragile).sum()) == 0, "the device and the restatement disagree"
        n_ground += int(mask.sum())
        n_fragile += int(fragile.sum())

    def run():
        return ground.estimate_ground_batch(dev, prm)
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
    print(json.dumps(dict(shape=shape_name, points=len(host[0]), us=statistics.median(ts), lo=min(ts), hi=max(ts), calls=len(names),
                          launches1=launches(host[:1]), launches8=launches(host), host_ms=statistics.median(hs), host_lo=min(hs),
                          host_hi=max(hs), ground=n_ground, fragile=n_fragile)))


def main():
    lines = ["| 8 scans of | path | time (median) | min – max | launches, batch 1 / batch 8 | C-ABI calls | ground points | fragile |",
             "|---|---|---|---|---|---|---|---|"]
    for shape_name, label in (("NUSCENES", "34,880 (nuScenes shape)"), ("KITTI", "120,000 (SemanticKITTI shape)")):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", shape_name], capture_output=True, text=True, timeout=LIMIT)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"{shape_name}: the measurement ended with status {out.returncode}")
        r = json.loads(out.stdout.strip().splitlines()[-1])
        assert r["launches1"] == r["launches8"], "the launch count depends on the batch size"
        lines.append(f"| {label} | estimate_ground_batch, device inputs | {r['us']:,.0f} µs | {r['lo']:,.0f} – {r['hi']:,.0f} µs | "
                     f"{r['launches1']} / {r['launches8']} | {r['calls']} | {r['ground']:,} | {r['fragile']} |")
        lines.append(f"| {label} | numpy restatement on the host, one thread | {r['host_ms']:,.0f} ms | {r['host_lo']:,.0f} – {r['host_hi']:,.0f} ms | | | | |")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one(sys.argv[2])
    else:
        main()
