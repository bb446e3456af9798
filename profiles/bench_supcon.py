#!/usr/bin/env python3
"""Supervised contrastive loss forward + backward on one GPU, two recipes on leaf features (unit-norm rows, 10 classes) in one process:

  (a) the loss of DESIGN.md section 4 evaluated by torch in float32 (restated here: S = A Q^T / T, the row maximum subtracted, a
      boolean positive mask, D = sum over the negatives of exp + 1e-5 through torch.where, mean over the positives minus log D) +
      autograd -- (Na, Nq) float32 arrays for S, the shifted logits, exp and the two selections, and a boolean mask
  (b) mopa_amd.models.losses.supcon_loss + backward (both gradients)

at (Na, Nq, F) = (1024, 8192, 16), (1024, 8192, 64), (4096, 65536, 16), (4096, 65536, 64).  HIP events around the Python call, median
of 50 after 5 warm-up calls; peak memory is torch.cuda.max_memory_allocated over a call less what was allocated before it.  Launches
are device kernels counted by torch.profiler in one extra, untimed call; the per-kernel times of (b) come from the same profile and
give each kernel's fraction of the 157.3 TFLOP/s f32 matrix peak: the forward at 2 Na Nq F flop, each backward at 4 Na Nq F (S again
and W X), 5 x 2 Na Nq F in total.

  python profiles/bench_supcon.py [--reps 50] [--out FILE.md] [--skip-torch-above BYTES]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mopa_amd import _lib  # noqa: E402
from mopa_amd.models.losses import supcon_loss  # noqa: E402

SHAPES = ((1024, 8192, 16), (1024, 8192, 64), (4096, 65536, 16), (4096, 65536, 64))
PEAK = 157.3e12


def torch_composite(la, a, q, lq, T=0.1):
    """The arithmetic of DESIGN.md section 4 as plain torch calls: a boolean positive mask, the shifted logits, E + eps |N| over the
    negatives, the mean over the positives."""
    S = (a @ q.t()) / T
    d = S - S.amax(dim=1, keepdim=True).detach()
    pos = la.view(-1, 1) == lq.view(1, -1)
    zero = torch.zeros((), dtype=d.dtype, device=d.device)
    D = torch.where(pos, zero, d.exp() + 1e-5).sum(dim=1)
    mean_pos = torch.where(pos, d, zero).sum(dim=1) / pos.sum(dim=1)
    return (D.log() - mean_pos).mean()


def step(fn, la, a, q, lq):
    a.grad = q.grad = None
    fn(la, a, q, lq).backward()


def timed(fn, args, reps):
    for _ in range(5):
        step(fn, *args)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        step(fn, *args)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def peak_bytes(fn, args):
    args[1].grad = args[2].grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(fn, *args)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def profile_once(fn, args):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step(fn, *args)
    torch.cuda.synchronize()
    kernels, per = 0, {}
    for e in prof.events():
        if str(getattr(e, "device_type", "")).endswith("CUDA"):
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                continue
            kernels += 1
            per[e.name] = per.get(e.name, 0.0) + (getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
    return kernels, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-torch-above", type=float, default=64e9, help="skip recipe (a) when 12 (Na, Nq) float32 arrays exceed this")
    a = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; forward + backward (both gradients), HIP events around the Python call, median of "
             f"{a.reps} (min - max) after 5 warm-up calls", "",
             "| Na | Nq | F | recipe | call µs | device kernels | peak memory over the call (MB) |", "|---|---|---|---|---|---|---|"]
    notes = []
    for Na, Nq, F in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(Na + F)
        A = torch.nn.functional.normalize(torch.randn(Na, F, device="cuda", generator=gen), dim=1).requires_grad_(True)
        Q = torch.nn.functional.normalize(torch.randn(Nq, F, device="cuda", generator=gen), dim=1).requires_grad_(True)
        la = torch.randint(0, 10, (Na,), device="cuda", generator=gen)
        lq = torch.randint(0, 10, (Nq,), device="cuda", generator=gen)
        args = [la, A, Q, lq]
        med = {}
        for name, fn in (("(a) torch composite, float32", torch_composite), ("(b) supcon_loss", supcon_loss)):
            if name.startswith("(a)") and 12.0 * Na * Nq * 4 > a.skip_torch_above:
                lines.append(f"| {Na:,} | {Nq:,} | {F} | {name} | does not fit the limit of {a.skip_torch_above / 1e9:.0f} GB | | |")
                continue
            t = timed(fn, args, a.reps)
            kernels, per = profile_once(fn, args)
            mem = peak_bytes(fn, args)
            med[name[:3]] = statistics.median(t)
            lines.append(f"| {Na:,} | {Nq:,} | {F} | {name} | {statistics.median(t):.1f} ({min(t):.1f} - {max(t):.1f}) | {kernels} | {mem / 1e6:.1f} |")
            print(lines[-1], flush=True)
            if name.startswith("(b)"):
                flop = 2.0 * Na * Nq * F
                pick = lambda key: sum(v for k, v in per.items() if key in k)     # noqa: E731
                fwd, b0, b1 = pick("k_supcon_fwd"), pick("k_supcon_bwd<0>"), pick("k_supcon_bwd<1>")
                frac = lambda us, n: 100.0 * n * flop / (us * 1e-6) / PEAK if us else float("nan")     # noqa: E731
                notes.append(f"* ({Na:,}, {Nq:,}, {F}): workspace {_lib.query('mopa_supcon_workspace_bytes', Na, Nq, F) / 1e6:.2f} MB, state "
                             f"{_lib.query('mopa_supcon_state_bytes', Na) / 1e3:.1f} kB, {_lib.query('mopa_supcon_pool_chunks', Na, Nq)} pool chunks; "
                             f"k_supcon_fwd {fwd:.1f} µs = {frac(fwd, 1):.1f} % of the f32 matrix peak, k_supcon_bwd<0> {b0:.1f} µs = {frac(b0, 2):.1f} %, "
                             f"k_supcon_bwd<1> {b1:.1f} µs = {frac(b1, 2):.1f} %; all kernels {sum(per.values()):.1f} µs = "
                             f"{frac(sum(per.values()), 5):.1f} % at 5 x 2 Na Nq F; per kernel: "
                             + ", ".join(f"{k.split('(')[0]} {v:.1f}" for k, v in sorted(per.items(), key=lambda kv: -kv[1])))
        if "(a)" in med:
            notes.append(f"  ratio (b) / (a) = {med['(b)'] / med['(a)']:.3f}: the device call is "
                         f"{'not slower' if med['(b)'] <= med['(a)'] else 'SLOWER'} than the torch sequence")
    text = "\n".join(lines) + "\n\nPer shape, recipe (b):\n\n" + "\n".join(notes) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
