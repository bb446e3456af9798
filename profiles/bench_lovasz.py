#!/usr/bin/env python3
"""Lovasz-softmax forward + backward on one GPU, recipes on leaf inputs in one process:

  (a) the reference's sequence of torch calls in float32, written out here (the boolean mask and gather of the valid rows with its
      nonzero(), then per class: mask, the `fg.sum() == 0` host read, torch.sort, gather, two cumulative sums, the Jaccard
      expression with its float32 difference, dot; the mean over the present classes) + autograd
  (b) mopa_amd.common.utils.loss.lovasz_softmax on the same probabilities + backward
  (c) lovasz_softmax_logits on logits + backward (against (a) behind torch.softmax, listed as (a'))

at (P, C) = (25,000, 10), (200,000, 10), (960,000, 10), (200,000, 5) with 30 % of the rows ignored.  HIP events around the Python call,
median of 50 after 5 warm-up calls.  Launches are device kernels counted by torch.profiler in one extra, untimed call; host
synchronisations are counted at torch.cuda.synchronize / Tensor.item / Tensor.__bool__ / Tensor.nonzero (Python level) and as
hipStreamSynchronize / hipDeviceSynchronize / hipEventSynchronize runtime events of that call, less those of an empty profiled
region.  From the same profile of (b): the sort kernels' (k_lov_hist + k_lov_rowscan + k_lov_scatter) time against the HBM floor of
8 bytes per pair read and 8 written per pass at 6.3 TB/s.

  python profiles/bench_lovasz.py [--reps 50] [--out FILE.md] [--device-only] [--passes N]

--device-only skips (a): for a library built with another digit width (lovasz.hip compiled with -DLOV_BITS=8, loaded through
MOPA_HIP_LIB); --passes is that build's pass count, for the floor (default 3, the 10-bit build).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mopa_amd.common.utils.loss import lovasz_softmax, lovasz_softmax_logits  # noqa: E402

SHAPES = ((25_000, 10), (200_000, 10), (960_000, 10), (200_000, 5))
IGNORE = 255
HBM = 6.3e12


def torch_composite(probas, labels):
    keep = labels != IGNORE
    p = probas[keep.nonzero().squeeze()]            # a host read (the row count of the result)
    y = labels[keep]
    per_class = []
    for c in range(p.shape[1]):
        member = (y == c).float()
        if member.sum() == 0:                       # a host read per class
            continue
        e, order = torch.sort((member - p[:, c]).abs(), 0, descending=True)
        m = member[order]
        total = m.sum()
        inter = total - m.cumsum(0)
        union = total + (1 - m).cumsum(0)
        j = 1. - inter / union
        j[1:] = j[1:] - j[:-1]                      # the float32 cancellation the device does in float64
        per_class.append(torch.dot(e, j))
    return sum(per_class) / len(per_class)


def torch_composite_logits(logits, labels):
    return torch_composite(torch.softmax(logits, 1), labels)


def device_logits(logits, labels):
    return lovasz_softmax_logits(logits, labels, ignore_index=IGNORE)


def device_probas(probas, labels):
    return lovasz_softmax(probas, labels, ignore=IGNORE)


def step(fn, x, y):
    x.grad = None
    if fn is not None:
        fn(x, y).backward()


def timed(fn, x, y, reps):
    for _ in range(5):
        step(fn, x, y)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        step(fn, x, y)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def profile_once(fn, x, y):
    """-> (device kernels, Python-level synchronisations, runtime synchronise calls, {kernel name: microseconds}) of one call (an
    empty `fn` gives the runtime calls of the profiler itself)."""
    from torch.profiler import ProfilerActivity, profile
    syncs = [0]
    saved = (torch.Tensor.item, torch.Tensor.__bool__, torch.cuda.synchronize, torch.Tensor.nonzero)

    def wrap(f):
        def g(*a, **k):
            syncs[0] += 1
            return f(*a, **k)
        return g
    torch.Tensor.item, torch.Tensor.__bool__, torch.cuda.synchronize, torch.Tensor.nonzero = (wrap(f) for f in saved)
    try:
        torch.cuda.synchronize()
        syncs[0] = 0
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(fn, x, y)
            python_syncs = syncs[0]   # before the profiler's own synchronize at the end of the region
    finally:
        torch.Tensor.item, torch.Tensor.__bool__, torch.cuda.synchronize, torch.Tensor.nonzero = saved
    torch.cuda.synchronize()
    kernels, per, runtime_syncs = 0, {}, 0
    for e in prof.events():
        if str(getattr(e, "device_type", "")).endswith("CUDA"):
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                continue
            kernels += 1
            per[e.name] = per.get(e.name, 0.0) + (getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
        elif e.name in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize"):
            runtime_syncs += 1
    return kernels, python_syncs, runtime_syncs, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; library {os.path.basename(os.environ.get('MOPA_HIP_LIB', '')) or 'as built'}; forward + backward, HIP "
             f"events around the Python call, median of {a.reps} (min - max) after 5 warm-up calls; microseconds", "",
             "| P | C | recipe | call µs | device kernels | host syncs (Python level) | runtime synchronise calls |",
             "|---|---|---|---|---|---|---|"]
    notes = []
    own = None
    recipes = (("(a) torch composite on probabilities, float32", torch_composite, False),
               ("(b) lovasz_softmax on probabilities", device_probas, False),
               ("(a') torch softmax + composite on logits, float32", torch_composite_logits, True),
               ("(c) lovasz_softmax_logits on logits", device_logits, True))
    for P, C in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(P + C)
        z = 3.0 * torch.randn(P, C, device="cuda", generator=gen)
        y = torch.randint(0, C, (P,), device="cuda", generator=gen)
        y = torch.where(torch.rand(P, device="cuda", generator=gen) < 0.3, torch.full_like(y, IGNORE), y)
        leaf = {False: torch.softmax(z, 1).requires_grad_(True), True: z.clone().requires_grad_(True)}
        med = {}
        for name, fn, logits in recipes:
            if a.device_only and name.startswith("(a"):
                continue
            x = leaf[logits]
            t = timed(fn, x, y, a.reps)
            if own is None:
                own = profile_once(None, x, y)[2]
                lines.insert(1, f"runtime synchronise calls of an empty profiled region (the profiler's own): {own}; subtracted below")
            kernels, syncs, rt_syncs, per = profile_once(fn, x, y)
            med[name.split(")")[0] + ")"] = statistics.median(t)
            lines.append(f"| {P:,} | {C} | {name} | {statistics.median(t):.1f} ({min(t):.1f} - {max(t):.1f}) | {kernels} | {syncs} | {rt_syncs - own} |")
            print(lines[-1], flush=True)
            if name.startswith("(b)") or name.startswith("(c)"):
                tot = sum(per.values())
                part = {k: sum(v for n, v in per.items() if k in n) for k in ("k_lov_count", "k_lov_hist", "k_lov_rowscan", "k_lov_scatter",
                                                                             "k_lov_fgcount", "k_lov_weights", "k_lov_final", "k_lov_bwd")}
                sort = part["k_lov_hist"] + part["k_lov_rowscan"] + part["k_lov_scatter"]
                floor_bytes = a.passes * 16 * P * C        # every class is present in these draws
                notes.append(f"* {name[:3]} ({P:,}, {C}): kernels sum to {tot:.1f} µs of device time; sort passes {sort:.1f} µs = "
                             f"{100 * floor_bytes / HBM / (sort * 1e-6):.1f} % of the HBM floor ({a.passes} passes x 16 B x {P * C:,} pairs = "
                             f"{floor_bytes / 1e6:.1f} MB at 6.3 TB/s = {floor_bytes / HBM * 1e6:.1f} µs); per kernel: "
                             + ", ".join(f"{k} {v:.1f}" for k, v in part.items())
                             + f"; others {tot - sum(part.values()):.1f}")
        if not a.device_only:
            for own_r, base in (("(b)", "(a)"), ("(c)", "(a')")):
                r = med[own_r] / med[base]
                notes.append(f"  ({P:,}, {C}): ratio {own_r} / {base} = {r:.3f}: the device call is {'not slower' if r <= 1 else 'SLOWER'} than the torch path")
    text = "\n".join(lines) + "\n\nPer shape, device recipes:\n\n" + "\n".join(notes) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
