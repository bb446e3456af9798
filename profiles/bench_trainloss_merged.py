#!/usr/bin/env python3
"""The loss block of a MERGED pass (source + target [+ the VGI batch] as row segments of one logit tensor per network), two
recipes on leaf logits in one process:

  (a) mopa_amd.trainloss.point_losses once per segment on row slices of the merged logits + backward of both loss sums (autograd
      pads every slice's gradient to the full tensor and adds it)
  (b) mopa_amd.trainloss.point_losses_merged over all segments + the same two backward calls

at 279,040 + 279,040 rows, C = 5 (8 + 8 nuScenes-shape scans) without and with a 3D-only third segment of 279,040 rows, and at
960,000 + 960,000 rows, C = 10 (8 + 8 SemanticKITTI-shape scans); dual head on and off.  The source segment has class weights, the
target segment pseudo labels without them, the third segment CE only.  As in profiles/bench_trainloss.py: ~10 ms of dummy device
work is enqueued before each timed phase; HOST = wall time from the first enqueue of the phase to the return of its last call,
DEVICE = HIP-event time from the end of the dummy work to the end of the phase; after a warm-up the recipes alternate; the table
gives min - max (median) over the rounds.  Launches: library entry-point calls counted at `call`, device kernels counted by
torch.profiler in one extra, untimed round per recipe.

  python profiles/bench_trainloss_merged.py [--rounds 7] [--kernels] [--out FILE.md]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mopa_amd import trainloss  # noqa: E402
from mopa_amd.trainloss import Segment, point_losses, point_losses_merged  # noqa: E402

# (rows per segment, C, third 3D-only segment, what)
SHAPES = ((279040, 5, False, "8 + 8 nuScenes scans"), (279040, 5, True, "8 + 8 nuScenes scans + VGI batch"),
          (960000, 10, False, "8 + 8 SemanticKITTI scans"))


def make_case(n, C, third, dual):
    gen = torch.Generator(device="cuda").manual_seed(n + C + int(third))
    N2, N3 = 2 * n, (3 if third else 2) * n
    rows = {"z2m": N2, "z2x": N2, "z3m": N3, "z3x": N3}
    names = ("z2m", "z2x", "z3m", "z3x") if dual else ("z2m", "z3m")
    L = {k: (torch.randn(rows[k], C, device="cuda", generator=gen) * 2).requires_grad_(True) for k in names}
    ys = []
    for _ in range(3 if third else 2):
        y = torch.randint(0, C, (n,), device="cuda", generator=gen)
        y[torch.rand(n, device="cuda", generator=gen) < 0.3] = -100
        ys.append(y)
    w = torch.rand(C, device="cuda", generator=gen) * 2 + 1
    p2, p3 = {"seg_logit": L["z2m"]}, {"seg_logit": L["z3m"]}
    if dual:
        p2["seg_logit2"], p3["seg_logit2"] = L["z2x"], L["z3x"]
    return L, p2, p3, ys, w, n


def _total(terms):
    terms = [t for t in terms if t is not None]
    return sum(terms[1:], terms[0])


def recipe_a(p2, p3, ys, w, n):
    res = []
    for s, y in enumerate(ys):
        q2 = {k: v[s * n:(s + 1) * n] for k, v in p2.items()} if s < 2 else None
        q3 = {k: v[s * n:(s + 1) * n] for k, v in p3.items()}
        res.append(point_losses(q2, q3, label=y, weight=w if s != 1 else None, kl=s < 2))
    _total([r.ce_2d for r in res] + [0.1 * r.kl_2d for r in res if r.kl_2d is not None]).backward()
    _total([r.ce_3d for r in res] + [0.1 * r.kl_3d for r in res if r.kl_3d is not None]).backward()


def recipe_b(p2, p3, ys, w, n):
    segs = [Segment(n, label=y, weighted=s != 1, kl=s < 2, in_2d=s < 2) for s, y in enumerate(ys)]
    res = point_losses_merged(p2, p3, segs, weight=w).segments
    _total([r.ce_2d for r in res] + [0.1 * r.kl_2d for r in res if r.kl_2d is not None]).backward()
    _total([r.ce_3d for r in res] + [0.1 * r.kl_3d for r in res if r.kl_3d is not None]).backward()


class Dummy:
    """A matmul chain sized once to ~`ms` of device time."""

    def __init__(self, ms=10.0):
        self.a = torch.randn(4096, 4096, device="cuda")
        self.b = torch.randn(4096, 4096, device="cuda")
        self.out = torch.empty_like(self.a)
        self.reps = 4
        for _ in range(3):
            t = self.time()
            self.reps = max(1, round(self.reps * ms / t))
        self.ms = self.time()

    def run(self):
        for _ in range(self.reps):
            torch.mm(self.a, self.b, out=self.out)

    def time(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self.run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)


def timed(fn, dummy, L, args):
    for t in L.values():
        t.grad = None
    torch.cuda.synchronize()
    dummy.run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn(*args)
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    torch.cuda.synchronize()
    return host, e0.elapsed_time(e1)


def launches(fn, L, args, count_kernels):
    """-> (library entry-point calls, device kernels or None) of one untimed run."""
    for t in L.values():
        t.grad = None
    names, inner = [], trainloss.call

    def call(name, *a):
        names.append(name)
        return inner(name, *a)
    trainloss.call = call
    kernels = None
    try:
        torch.cuda.synchronize()
        if count_kernels:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn(*args)
                torch.cuda.synchronize()
            kernels = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")) or None
        else:
            fn(*args)
    finally:
        trainloss.call = inner
    torch.cuda.synchronize()
    return len(names), kernels


def fmt(v):
    return f"{min(v):.2f} - {max(v):.2f} ({statistics.median(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true", help="count device kernels with torch.profiler in an extra round")
    a = ap.parse_args()
    assert a.rounds >= 5
    dummy = Dummy()
    lines = [f"device: {torch.cuda.get_device_name(0)}; dummy work in front of every phase: {dummy.reps} x mm(4096) = {dummy.ms:.1f} ms; "
             f"{a.rounds} alternating rounds after 3 warm-up rounds; ms, min - max (median)", "",
             "| rows per segment | segments | C | dual head | recipe | host ms | device ms | library calls | device kernels |",
             "|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for n, C, third, what in SHAPES:
        for dual in (True, False):
            L, p2, p3, ys, w, n = make_case(n, C, third, dual)
            res = {"a": ([], []), "b": ([], [])}
            for rnd in range(3 + a.rounds):
                for name, fn in (("a", recipe_a), ("b", recipe_b)):
                    host, dev = timed(fn, dummy, L, (p2, p3, ys, w, n))
                    if rnd >= 3:
                        res[name][0].append(host)
                        res[name][1].append(dev)
            count = {name: launches(fn, L, (p2, p3, ys, w, n), a.kernels) for name, fn in (("a", recipe_a), ("b", recipe_b))}
            for name in ("a", "b"):
                lib_calls, kernels = count[name]
                lines.append(f"| {n:,} ({what}) | {len(ys)} | {C} | {'on' if dual else 'off'} | ({name}) | {fmt(res[name][0])} | "
                             f"{fmt(res[name][1])} | {lib_calls} | {'not counted' if kernels is None else kernels} |")
            da, db = res["a"][1], res["b"][1]
            limit = statistics.median(da) + (max(da) - min(da))
            fewer = count["b"][0] < count["a"][0] and (count["a"][1] is None or count["b"][1] is None or count["b"][1] < count["a"][1])
            print(lines[-2], lines[-1], sep="\n", flush=True)
            verdicts.append(f"* {n:,} x {len(ys)}, C = {C}, dual head {'on' if dual else 'off'}: (b) device median {statistics.median(db):.3f} ms; "
                            f"limit = (a) median {statistics.median(da):.3f} + (a) spread {max(da) - min(da):.3f} = {limit:.3f} ms: "
                            f"{'met' if statistics.median(db) <= limit else 'NOT met'}; fewer launches: {'yes' if fewer else 'NO'}")
    text = "\n".join(lines) + "\n\nAcceptance per row pair:\n\n" + "\n".join(verdicts) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
