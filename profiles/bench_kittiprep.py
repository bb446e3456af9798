#!/usr/bin/env python3
"""prepare_scans_kitti (mopa_amd/kittiprep.py, csrc/kittiprep.hip) at 2 + 2 and 8 + 8 scans of 120,000 points, image 1226 x 370,
ground index lists of a third of the points, with_full on: HIP-event time around one call with resident inputs (host enqueue and
the one read-back included), median of 50 after 5 warm-up calls; C-ABI calls per call; achieved bandwidth on the algorithmic
bytes (scan, labels and ground lists in once; every returned array out) beside 6.3 TB/s.

Beside it the same work in numpy on the host of the GPU machine: a restatement of the dataset's expressions (the z filter, the low 16
bits, the ground mask, the front half, the float32 matmul, the divide, np.around, the frustum test, the boolean compactions) for
the same scans on one thread, median of 3.  Writes a markdown table to stdout (and to argv[1] if given)."""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from mopa_amd import _lib, kittiprep as kp  # noqa: E402

HBM = 6.3e12
SIZE = (1226, 370)
P2 = np.array([[718.856, 0, 607.1928, 45.38225], [0, 718.856, 185.2157, -0.1130887], [0, 0, 1, 0.003779761]])
TR = np.array([[4.276802385584e-04, -9.999672484946e-01, -8.084491683471e-03, -1.198459927713e-02],
               [-7.210626507497e-03, 8.081198471645e-03, -9.999413164504e-01, -5.403984729748e-02],
               [9.999738645903e-01, 4.859485810390e-04, -7.206933692422e-03, -2.921968648686e-01], [0, 0, 0, 1]])


def make(B, n=120000, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(B):
        scan = np.stack([rng.uniform(-70, 70, n), rng.uniform(-70, 70, n), rng.uniform(-3.4, 2, n), rng.random(n)], 1).astype(np.float32)
        label = ((rng.integers(0, 1 << 16, n).astype(np.uint32) << 16) | rng.integers(0, 260, n).astype(np.uint32)).view(np.int32)
        out.append({"scan": scan, "label": label, "proj_matrix": P2 @ TR, "g_indices": np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)})
    return out


def host_path(samples):
    """The dataset's per-sample expressions in numpy.  -> [(Nz, Nk)]"""
    counts = []
    for s in samples:
        scan = s["scan"]
        points, feats = scan[:, :3], scan[:, 3]
        label = s["label"].view(np.uint32) & 0xFFFF
        z_idx = points[:, 2] > -3
        points, feats, label = points[z_idx], feats[z_idx], label[z_idx]
        g_mask = np.zeros(scan.shape[0])
        g_mask[s["g_indices"]] = 1
        g_mask = g_mask[z_idx].astype(np.bool_)
        seg, all_seg = label.astype(np.int16), label.astype(np.int16)
        keep_idx = points[:, 0] > 0
        h = np.concatenate([points[keep_idx], np.ones([keep_idx.sum(), 1], dtype=np.float32)], axis=1)
        img = np.matmul(s["proj_matrix"].astype(np.float32), h.T, dtype=np.float32).T
        img = img[:, :2] / np.expand_dims(img[:, 2], axis=1)
        img = np.around(img, decimals=2)
        k2 = (img[:, 0] > 0) * (img[:, 1] > 0) * (img[:, 0] < SIZE[0]) * (img[:, 1] < SIZE[1])
        keep_idx[keep_idx] = k2
        img = np.fliplr(img[k2])
        out = (points[keep_idx], feats[keep_idx].reshape(-1, 1), seg[keep_idx], img, g_mask[keep_idx], all_seg)
        counts.append((len(points), len(out[0])))
    return counts


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
    lines = ["| batch | path | µs (median) | min – max | C-ABI calls | algorithmic MB | GB/s | of 6.3 TB/s |", "|---|---|---|---|---|---|---|---|"]
    torch.set_num_threads(1)
    for B in (4, 16):
        host = make(B)
        dev = [{k: (torch.from_numpy(v).cuda() if k != "proj_matrix" else v) for k, v in s.items()} for s in host]

        def run():
            return kp.prepare_scans_kitti(dev, SIZE, with_full=True)
        names = []
        orig = _lib.call
        kp.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
        res = run()
        kp.call = orig
        want = host_path(host)
        assert [tuple(c) for c in res["counts"].tolist()] == want, "the device and the numpy restatement disagree on the counts"
        nz, nk = (int(v) for v in res["counts"].sum(0))
        byts = sum(16 * len(s["scan"]) + 4 * len(s["scan"]) + 4 * len(s["g_indices"]) for s in host) + nz * (1 + 12 + 2) + nk * (12 + 4 + 2 + 8 + 1)
        med, lo, hi = timed(run)
        lines.append(f"| {B // 2} + {B // 2} x 120,000 | prepare_scans_kitti, with_full, ground lists | {med:,.1f} | {lo:,.1f} – {hi:,.1f} | {len(names)} | "
                     f"{byts / 1e6:.1f} | {byts / med / 1e3:,.0f} | {byts / (med * 1e-6) / HBM:.3f} |")
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_path(host)
            hs.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"| {B // 2} + {B // 2} x 120,000 | numpy on the host, one thread | {statistics.median(hs):,.1f} | {min(hs):,.1f} – {max(hs):,.1f} | | | | |")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
