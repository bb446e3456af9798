#!/usr/bin/env python3
"""evaluate_batch (csrc/evaluate.hip) against (a) the same math as torch device ops and (b) the reference's host path, at three
validation shapes.  HIP-event times, median of 50 (b: of 5).  Writes a markdown table to stdout (and to argv[1] if given).

Effective bandwidth = (2 N C 4 + 8 N + outputs) bytes / time, against 6.3 TB/s achievable HBM.
(b) = what validate.py:112-157 does per batch: three argmax(...).cpu().numpy() copies, then per scan three
sklearn.metrics.confusion_matrix calls (numpy restatement when sklearn is absent), plus the entropy means and CE as torch ops.
"""
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from mopa_amd.evaluate import Evaluator, evaluate_batch  # noqa: E402

HBM = 6.3e12
SHAPES = [("32 nuScenes scans", 32, 34_880, 5), ("32 KITTI scans", 32, 120_000, 10), ("1 KITTI scan (batch 1)", 1, 120_000, 10)]

try:
    from sklearn.metrics import confusion_matrix as sk_cm
except ImportError:
    sk_cm = None


def cm_host(gt, pred, L):
    if sk_cm is not None:
        return sk_cm(gt, pred, labels=np.arange(L))
    keep = (gt >= 0) & (gt < L) & (pred >= 0) & (pred < L)
    return np.bincount(gt[keep] * L + pred[keep], minlength=L * L).reshape(L, L)


def torch_device(l2, l3, label, L):
    """(a): the same metrics as torch device ops; masked bincount; the ignore mask makes it sync (boolean indexing)."""
    p2, p3 = F.softmax(l2, 1), F.softmax(l3, 1)
    preds = (l2.argmax(1), l3.argmax(1), (p2 + p3).argmax(1))
    keep = (label >= 0) & (label < L)
    gt = label[keep]
    mats = [torch.bincount(gt * L + p[keep], minlength=L * L).view(L, L) for p in preds]
    c = l2.shape[1]
    ety = [(-(q * torch.log2(q + 1e-30)) / np.log2(c)).mean() for q in (F.softmax(p2, 1), F.softmax(p3, 1))]
    ce = [F.cross_entropy(l2, label), F.cross_entropy(l3, label)]
    return mats, ety, ce


def host_path(l2, l3, label, lens, L):
    """(b): the reference's host path."""
    pred2 = l2.argmax(1).cpu().numpy()
    pred3 = l3.argmax(1).cpu().numpy()
    p2, p3 = F.softmax(l2, 1), F.softmax(l3, 1)
    predx = (p2 + p3).argmax(1).cpu().numpy()
    c = l2.shape[1]
    e2 = (-(F.softmax(p2, 1) * torch.log2(F.softmax(p2, 1) + 1e-30)) / np.log2(c)).mean().item()
    e3 = (-(F.softmax(p3, 1) * torch.log2(F.softmax(p3, 1) + 1e-30)) / np.log2(c)).mean().item()
    gt_all = label.cpu().numpy()
    mats = [np.zeros((L, L)) for _ in range(3)]
    left = 0
    for m in lens:
        gt = gt_all[left:left + m].copy()
        gt[gt == -100] = L
        for k, p in enumerate((pred2, pred3, predx)):
            mats[k] += cm_host(gt, p[left:left + m], L)
        left += m
    ce = (F.cross_entropy(l2, label).item(), F.cross_entropy(l3, label).item())
    return mats, e2, e3, ce


def time_it(fn, reps, warm=3):
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
    return statistics.median(ts)


def main():
    rows = []
    for name, scans, per, c in SHAPES:
        n = scans * per
        g = torch.Generator().manual_seed(n)
        l2, l3 = (torch.randn(n, c, generator=g) * 3).cuda(), (torch.randn(n, c, generator=g) * 3).cuda()
        label = torch.randint(0, c, (n,), generator=g)
        label[torch.rand(n, generator=g) < 0.1] = -100
        label = label.cuda()
        names = [str(i) for i in range(c)]
        evs = {k: Evaluator(names) for k in ("2D", "3D", "2D+3D")}
        for pselab in (False, True):
            us = time_it(lambda: evaluate_batch(l2, l3, label, evaluators=evs, pselab=pselab), 50)
            out_bytes = 3 * c * c * 8 * 2 + (2 * n * 5 if pselab else 0)
            gbps = (2 * n * c * 4 + 8 * n + out_bytes) / (us * 1e-6)
            rows.append((name if not pselab else name + ", pselab", n, c, "evaluate_batch", us, gbps / 1e9, gbps / HBM))
        us_a = time_it(lambda: torch_device(l2, l3, label, c), 50)
        rows.append((name, n, c, "(a) torch device ops", us_a, None, None))
        us_b = time_it(lambda: host_path(l2, l3, label, [per] * scans, c), 5, warm=1)
        rows.append((name, n, c, "(b) host path (sklearn)" if sk_cm else "(b) host path (numpy)", us_b, None, None))
        # same counts as the host path
        ev = {k: Evaluator(names) for k in ("2D", "3D", "2D+3D")}
        evaluate_batch(l2, l3, label, evaluators=ev)
        mats = host_path(l2, l3, label, [per] * scans, c)[0]
        same = all(np.array_equal(ev[k].confusion_matrix, m) for k, m in zip(("2D", "3D"), mats[:2]))
        rows.append((name, n, c, f"2D/3D matrices equal to (b): {same}; xM cells differing: "
                     f"{int(np.abs(ev['2D+3D'].confusion_matrix - mats[2]).sum())}", 0.0, None, None))
    lines = ["| shape | N | C | path | µs (median) | GB/s | of 6.3 TB/s |", "|---|---|---|---|---|---|---|"]
    for name, n, c, path, us, gb, frac in rows:
        lines.append(f"| {name} | {n:,} | {c} | {path} | {us:,.1f} | {'' if gb is None else f'{gb:,.0f}'} | "
                     f"{'' if frac is None else f'{frac:.2f}'} |")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
