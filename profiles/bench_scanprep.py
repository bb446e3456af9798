#!/usr/bin/env python3
"""prepare_batch_3d (mopa_amd/scanprep.py, csrc/scanprep.hip) at B = 8 + 8 scans of 34,880 and of 120,000 points, ema_input on:
HIP-event time around one call with resident inputs (host enqueue included), median of 50 after 5 warm-up calls; with and without
pseudo labels; the assume_inside form and the general form; C-ABI calls and kernel launches per call; achieved bandwidth on the
algorithmic bytes (points, labels, indices, probabilities in; every returned array out) beside 6.3 TB/s -- as a description: the
call is launch-bound.

Against the per-scan path that exists without scanprep, for the same outputs (voxelize_scan with the rotation per scan and per
un-augmented copy, torch boolean indexing for the side arrays, one pseudo.refine_pseudo_labels per scan and array): three
alternating repetitions of both medians.  Against the host path: a numpy / torch-CPU restatement of the datasets' expressions for the
same 16 samples on one thread, median of 3.  Writes a markdown table to stdout (and to argv[1] if given)."""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from mopa_amd import _lib, scanprep as sp  # noqa: E402
from mopa_amd.pseudo import refine_pseudo_labels  # noqa: E402
from mopa_amd.voxelize import rotate_points, voxelize_scan  # noqa: E402

HBM = 6.3e12
CLASSES = 11
AUG = dict(noisy_rot=0.1, flip_x=0.5, flip_y=0.0, rot_z=6.2831, transl=True)


def make(n, B=16, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    np.random.seed(seed)
    out = []
    for b in range(B):
        q = (rng.standard_normal((n, 3)) * np.array([20.0, 20.0, 1.5])).astype(np.float32)
        if b % 2:
            q[:11, 2] = np.abs(q[:11, 2]) * 40 + 250
        rot, u = sp.draw_augmentation_3d(**AUG)
        out.append({"points": q, "rot": rot, "transl_u": u, "seg_label": rng.integers(0, 40, n).astype(np.uint8),
                    "img_indices": np.stack([rng.integers(0, 225, n), rng.integers(0, 400, n)], 1).astype(np.int64),
                    "pseudo_label_2d": rng.integers(0, CLASSES, n).astype(np.int32), "probs_2d": rng.random(n, dtype=np.float32),
                    "pseudo_label_3d": rng.integers(0, CLASSES, n).astype(np.int32), "probs_3d": rng.random(n, dtype=np.float32)})
    mapping = rng.integers(0, CLASSES, 40).astype(np.int64)
    mapping[::7] = -100
    return out, mapping


def parent_path(samples, mapping, pseudo):
    """The same outputs scan by scan with what exists without scanprep."""
    locs, ori, seg, img, aug, ps2, ps3, ori_ps = [], [], [], [], [], [], [], []
    for b, s in enumerate(samples):
        c, keep = voxelize_scan(s["points"], 20, 4096, s["transl_u"], b, rot=s["rot"])
        oc, _ = voxelize_scan(s["points"], 20, 4096, None, b)
        locs.append(c)
        ori.append(oc)
        seg.append(mapping[s["seg_label"].long()][keep])
        img.append(s["img_indices"][keep])
        aug.append(rotate_points(s["points"], s["rot"])[keep])
        if pseudo:
            r2 = refine_pseudo_labels(s["probs_2d"], s["pseudo_label_2d"], num_classes=CLASSES)
            r3 = refine_pseudo_labels(s["probs_3d"], s["pseudo_label_3d"], num_classes=CLASSES)
            ps2.append(r2[keep])
            ps3.append(r3[keep])
            ori_ps.append(r3)
    locs, ori = torch.cat(locs), torch.cat(ori)
    out = {"x": [locs, torch.ones(locs.shape[0], 1, device=locs.device)], "ori_x": [ori, torch.ones(ori.shape[0], 1, device=ori.device)],
           "seg_label": torch.cat(seg), "img_indices": img, "aug_points_ls": aug}
    if pseudo:
        out.update({"pseudo_label_2d": torch.cat(ps2), "pseudo_label_3d": torch.cat(ps3), "ori_pslabel_ls": ori_ps})
    return out


def host_path(samples, mapping, pseudo):
    """The datasets' per-sample expressions on one thread (numpy; the refinement with torch on the CPU as the reference does)."""
    def refine(probs, lab):
        probs, lab = torch.tensor(probs), torch.tensor(lab)
        for c in lab.unique():
            idx = torch.nonzero(lab == c).squeeze(1)
            thresh = min(probs[idx].median(), 0.9)
            lab[idx[probs[idx] < thresh]] = -100
        return lab.numpy()

    def vox(p, u):
        c = np.round(p * 20)
        c -= c.min(0)
        if u is not None:
            c += np.clip(4096 - c.max(0) - 0.001, a_min=0, a_max=None) * u
        return c

    for s in samples:
        seg = mapping[s["seg_label"]]
        p = s["points"].dot(s["rot"])
        c = vox(p, s["transl_u"]).astype(np.int64)
        idxs = (c.min(1) >= 0) * (c.max(1) < 4096)
        c[idxs], p[idxs], seg[idxs], s["img_indices"][idxs]
        oc = vox(s["points"], None)
        oc[(oc.min(1) >= 0) * (oc.max(1) < 4096)]
        if pseudo:
            refine(s["probs_2d"], s["pseudo_label_2d"].astype(np.int32))[idxs]
            refine(s["probs_3d"], s["pseudo_label_3d"].astype(np.int32))[idxs]


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
    return statistics.median(ts)


def launches(names, n, general, pseudo):
    """Kernels behind the entry points of one call (memsets not counted)."""
    rows = _lib.query("mopa_scanprep_rows_per_block")
    nblk = 2 * 16 * -(-n // rows)
    per = {"mopa_scanprep_rotate": 1, "mopa_scanprep_count": 2 + ((2 + (1 if 2 * nblk + 1 <= 8192 else 3)) if general else 0),
           "mopa_scanprep_compact": 1, "mopa_scanprep_take": 1, "mopa_refine_pseudo_labels_segmented": 9}
    return sum(per[nm] for nm in names)


def main():
    lines = ["| batch | path | µs (median) | C-ABI calls | kernels | algorithmic MB | GB/s | of 6.3 TB/s |", "|---|---|---|---|---|---|---|---|"]
    ab = []
    for n in (34880, 120000):
        host, mapping = make(n)
        dev = [{k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) and k not in ("rot", "transl_u") else v) for k, v in s.items()}
               for s in host]
        mp = torch.from_numpy(mapping).cuda()
        for pseudo in (False, True):
            samples = dev if pseudo else [{k: v for k, v in s.items() if "pseudo" not in k and "probs" not in k} for s in dev]
            for inside in (True, False):
                def run():
                    return sp.prepare_batch_3d(samples, 20, 4096, label_mapping=mp, ema_input=True, assume_inside=inside, num_classes=CLASSES)
                names = []
                orig = _lib.call
                sp.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
                run()
                sp.call = orig
                us = timed(run)
                byts = 16 * n * (12 + 1 + 16 + 32 + 4 + 8 + 16 + 12 + 8 + 1 + 32 + 4 + (2 * 8 + 3 * 8 if pseudo else 0))
                form = "assume_inside" if inside else "general"
                lines.append(f"| 8 + 8 x {n:,} | prepare_batch_3d, {form}, {'with' if pseudo else 'no'} pseudo labels | {us:,.1f} | {len(names)} | "
                             f"{launches(names, n, not inside, pseudo)} | {byts / 1e6:.1f} | {byts / us / 1e3:,.0f} | {byts / (us * 1e-6) / HBM:.3f} |")
        for rep in range(3):           # alternating: the new call, then the per-scan path, same inputs
            new = timed(lambda: sp.prepare_batch_3d(dev, 20, 4096, label_mapping=mp, ema_input=True, num_classes=CLASSES))
            old = timed(lambda: parent_path(dev, mp, True), warm=3, n=20)
            ab.append(f"| 8 + 8 x {n:,} | repetition {rep + 1} | {new:,.1f} | {old:,.1f} | {old / new:.2f} |")
        torch.set_num_threads(1)
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_path(host, mapping, True)
            hs.append((time.perf_counter() - t0) * 1e6)
        lines.append(f"| 8 + 8 x {n:,} | host path (numpy, torch CPU; one thread), with pseudo labels | {statistics.median(hs):,.1f} | | | | | |")
    text = "\n".join(lines + ["", "| batch | general form with pseudo labels | prepare_batch_3d µs | per-scan path µs | ratio |", "|---|---|---|---|---|"] + ab)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
