#!/usr/bin/env python3
"""logCORAL forward + backward on one GPU, two recipes on leaf features in one process:

  (a) the reference's expression evaluated by torch in float32 (written out here from the formula: centre, covariances with the
      shared factor, the > 1e30 / NaN guard with its host reads, SVD, V diag(log e) V^T, mean squared difference) + autograd
  (b) mopa_amd.models.losses.logcoral_loss + backward

at (25,000, 25,000) and (100,000, 100,000) rows for F = 16 and F = 64.  HIP events around the Python call, median of 50 after 5
warm-up calls.  Launches are device kernels counted by torch.profiler in one extra, untimed call; host synchronisations are counted
at torch.cuda.synchronize / Tensor.item / Tensor.__bool__ (Python level) and as hipStreamSynchronize / hipDeviceSynchronize /
hipEventSynchronize runtime events of that call, less those of an empty profiled region.  The per-kernel times of (b) come from the same profile: the share of the eigen stage (k_coral_eigen + k_coral_loss) in the
call and the Gram and backward kernels' fraction of 6.3 TB/s on their floor traffic (one read of the input; one read and one write).

  python profiles/bench_logcoral.py [--reps 50] [--out FILE.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mopa_amd.models.losses import logcoral_loss  # noqa: E402

SHAPES = ((25_000, 25_000, 16), (25_000, 25_000, 64), (100_000, 100_000, 16), (100_000, 100_000, 64))
HBM = 6.3e12


def torch_composite(xs, xt):
    n = xs.shape[0]
    xs = xs.flatten(end_dim=-2) if xs.dim() > 2 else xs
    xt = xt.flatten(end_dim=-2) if xt.dim() > 2 else xt
    xs = xs - xs.mean(0)
    xt = xt - xt.mean(0)
    f = 1.0 / (n - 1)
    cs, ct = f * xs.t() @ xs, f * xt.t() @ xt
    bad = bool((cs > 1e30).any()) or bool((ct > 1e30).any()) or bool(torch.isnan(cs).any()) or bool(torch.isnan(ct).any())
    if bad:
        cs, ct = torch.eye(cs.shape[0], device=cs.device), torch.eye(ct.shape[0], device=ct.device)
    logs = []
    for c in (cs, ct):
        _, e, v = torch.svd(c)
        logs.append(v @ torch.diag(torch.log(e)) @ v.t())
    return ((logs[0] - logs[1]) ** 2).mean()


def step(fn, xs, xt):
    xs.grad = xt.grad = None
    if fn is not None:
        fn(xs, xt).backward()


def timed(fn, xs, xt, reps):
    for _ in range(5):
        step(fn, xs, xt)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        step(fn, xs, xt)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def profile_once(fn, xs, xt):
    """-> (device kernels, Python-level synchronisations, runtime synchronise calls, {kernel name: microseconds}) of one call (an
    empty `fn` gives the runtime calls of the profiler itself)."""
    from torch.profiler import ProfilerActivity, profile
    syncs = [0]
    saved = (torch.Tensor.item, torch.Tensor.__bool__, torch.cuda.synchronize)

    def wrap(f):
        def g(*a, **k):
            syncs[0] += 1
            return f(*a, **k)
        return g
    torch.Tensor.item, torch.Tensor.__bool__, torch.cuda.synchronize = wrap(saved[0]), wrap(saved[1]), wrap(saved[2])
    try:
        torch.cuda.synchronize()
        syncs[0] = 0
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(fn, xs, xt)
            python_syncs = syncs[0]   # before the profiler's own synchronize at the end of the region
    finally:
        torch.Tensor.item, torch.Tensor.__bool__, torch.cuda.synchronize = saved
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
    a = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; forward + backward, HIP events around the Python call, median of {a.reps} "
             "(min - max) after 5 warm-up calls; microseconds", "",
             "| rows (src, trg) | F | recipe | call µs | device kernels | host syncs (Python level) | runtime synchronise calls |",
             "|---|---|---|---|---|---|---|"]
    notes = []
    own = None
    for ns, nt, F in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(ns + F)
        mix = torch.randn(F, F, device="cuda", generator=gen)
        xs = (torch.randn(ns, F, device="cuda", generator=gen) @ mix).requires_grad_(True)
        xt = (torch.randn(nt, F, device="cuda", generator=gen) @ mix.t()).requires_grad_(True)
        med = {}
        for name, fn in (("(a) torch composite, float32", torch_composite), ("(b) logcoral_loss, float64", logcoral_loss)):
            t = timed(fn, xs, xt, a.reps)
            if own is None:
                own = profile_once(None, xs, xt)[2]
                lines.insert(1, f"runtime synchronise calls of an empty profiled region (the profiler's own): {own}; subtracted below")
            kernels, syncs, rt_syncs, per = profile_once(fn, xs, xt)
            med[name[:3]] = statistics.median(t)
            lines.append(f"| {ns:,}, {nt:,} | {F} | {name} | {statistics.median(t):.1f} ({min(t):.1f} - {max(t):.1f}) | {kernels} | {syncs} | {rt_syncs - own} |")
            print(lines[-1], flush=True)
            if name.startswith("(b)"):
                tot = sum(per.values())
                eig = sum(v for k, v in per.items() if "k_coral_eigen" in k or "k_coral_loss" in k)
                gram = sum(v for k, v in per.items() if "k_coral_gram" in k)
                bwd = sum(v for k, v in per.items() if "k_coral_bwd" in k)
                colsum = sum(v for k, v in per.items() if "k_coral_colsum" in k)
                gb_gram, gb_bwd = (ns + nt) * F * 4, 2 * (ns + nt) * F * 4
                notes.append(f"* {ns:,} + {nt:,} rows, F = {F}: kernels sum to {tot:.1f} µs of device time; eigen stage (k_coral_eigen + "
                             f"k_coral_loss) {eig:.1f} µs = {100 * eig / tot:.0f} %; k_coral_colsum {colsum:.1f} µs; k_coral_gram {gram:.1f} µs = "
                             f"{100 * gb_gram / (gram * 1e-6) / HBM:.1f} % of 6.3 TB/s on {gb_gram / 1e6:.1f} MB; k_coral_bwd (two launches) {bwd:.1f} µs = "
                             f"{100 * gb_bwd / (bwd * 1e-6) / HBM:.1f} % on {gb_bwd / 1e6:.1f} MB; per kernel: "
                             + ", ".join(f"{k.split('(')[0]} {v:.1f}" for k, v in sorted(per.items(), key=lambda kv: -kv[1])))
        notes.append(f"  ratio (b) / (a) = {med['(b)'] / med['(a)']:.3f}: the device call is {'not slower' if med['(b)'] <= med['(a)'] else 'SLOWER'} "
                     "than the torch composite")
    text = "\n".join(lines) + "\n\nPer shape, recipe (b):\n\n" + "\n".join(notes) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
