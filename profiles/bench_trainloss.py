#!/usr/bin/env python3
"""The loss-and-metric block of one domain half, two recipes in one process:

  (a) seg_ce x2 + xm_kl x2 + SegIoU.update_dict x2 + backward of both loss sums into leaf logits (the recipe before point_losses)
  (b) mopa_amd.trainloss.point_losses (with both SegIoU metrics) + the same two backward calls

at N = 279,040, C = 5 (8 nuScenes-shape scans) and N = 960,000, C = 10 (8 SemanticKITTI-shape scans), dual head on and off.  Before
each timed phase ~10 ms of dummy device work is enqueued, so that a host sync inside the phase has a queue to drain, as in a
training step.  Per phase: HOST = wall time from the first enqueue of the phase to the return of its last call (enqueue plus any
wait; the dummy work is enqueued before the clock starts), DEVICE = HIP-event time from the end of the dummy work to the end of the
phase.  After a warm-up the recipes alternate; the table gives min - max (median) over the rounds.

  python profiles/bench_trainloss.py [--rounds 7] [--out FILE.md]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mopa_amd.common.utils.loss import seg_ce, xm_kl  # noqa: E402
from mopa_amd.models.metric import SegIoU  # noqa: E402
from mopa_amd.trainloss import point_losses  # noqa: E402

SHAPES = ((279040, 5, "8 nuScenes scans"), (960000, 10, "8 SemanticKITTI scans"))


def make_case(N, C, dual):
    gen = torch.Generator(device="cuda").manual_seed(N + C)
    names = ("z2m", "z2x", "z3m", "z3x") if dual else ("z2m", "z3m")
    L = {k: (torch.randn(N, C, device="cuda", generator=gen) * 2).requires_grad_(True) for k in names}
    y = torch.randint(0, C, (N,), device="cuda", generator=gen)
    y[torch.rand(N, device="cuda", generator=gen) < 0.3] = -100
    w = torch.rand(C, device="cuda", generator=gen) * 2 + 1
    p2, p3 = {"seg_logit": L["z2m"]}, {"seg_logit": L["z3m"]}
    if dual:
        p2["seg_logit2"], p3["seg_logit2"] = L["z2x"], L["z3x"]
    return L, p2, p3, y, w


def recipe_a(p2, p3, y, w, m2, m3):
    x2, x3 = p2.get("seg_logit2", p2["seg_logit"]), p3.get("seg_logit2", p3["seg_logit"])
    loss_2d = [seg_ce(p2["seg_logit"], y, w), 0.1 * xm_kl(x2, p3["seg_logit"])]
    loss_3d = [seg_ce(p3["seg_logit"], y, w), 0.1 * xm_kl(x3, p2["seg_logit"])]
    with torch.no_grad():
        m2.update_dict(p2, {"seg_label": y})
        m3.update_dict(p3, {"seg_label": y})
    sum(loss_2d).backward()
    sum(loss_3d).backward()


def recipe_b(p2, p3, y, w, m2, m3):
    r = point_losses(p2, p3, label=y, weight=w, metric_2d=m2, metric_3d=m3)
    (r.ce_2d + 0.1 * r.kl_2d).backward()
    (r.ce_3d + 0.1 * r.kl_3d).backward()


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


def fmt(v):
    return f"{min(v):.2f} - {max(v):.2f} ({statistics.median(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    dummy = Dummy()
    lines = [f"device: {torch.cuda.get_device_name(0)}; dummy work in front of every phase: {dummy.reps} x mm(4096) = {dummy.ms:.1f} ms; "
             f"{a.rounds} alternating rounds after 3 warm-up rounds; ms, min - max (median)", "",
             "| N | C | dual head | recipe | host ms | device ms |", "|---|---|---|---|---|---|"]
    for N, C, what in SHAPES:
        for dual in (True, False):
            L, p2, p3, y, w = make_case(N, C, dual)
            res = {"a": ([], []), "b": ([], [])}
            for rnd in range(3 + a.rounds):
                for name, fn in (("a", recipe_a), ("b", recipe_b)):
                    host, dev = timed(fn, dummy, L, (p2, p3, y, w, SegIoU(C), SegIoU(C)))
                    if rnd >= 3:
                        res[name][0].append(host)
                        res[name][1].append(dev)
            for name in ("a", "b"):
                lines.append(f"| {N:,} ({what}) | {C} | {'on' if dual else 'off'} | ({name}) | {fmt(res[name][0])} | {fmt(res[name][1])} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
