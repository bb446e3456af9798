#!/usr/bin/env python3
"""The teacher phase of one MoPA iteration (train_xmuda_mopa.py:264-335), measured: host enqueue time (the call returns; nothing
is waited for) and device time between two HIP events, for 8 target scans of 302 x 480 / 34,880 points and for batch 1.

Legs (public API only):
  byhand   FlatEMA.average_parameters() + one model_2d call per image + model_3d + pseudo.pseudo_labels + scanprep.take --
           INTEGRATION.md's recipe before mopa_amd.teacher; runs unchanged on a commit without that module
  eager    Teacher(replay=False).pseudo_labels
  replay   Teacher().pseudo_labels (the 2D backbone as a replayed command list)
  perimg   Teacher().pseudo_labels(batched=False): the replayed pass, one image at a time like the reference

    python profiles/bench_teacher.py [--legs byhand,eager,replay,perimg] [--scans 8,1] [--iters 20] [--warmup 5] [--out FILE.json]

Between two measured calls one student-side event is simulated the way an iteration has it: ema.update() (the shadow -- and with it
every derived weight form of the teacher -- changes each iteration)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402


def build(scans):
    from mopa_amd import synth
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d, build_model_3d
    from mopa_amd.optim import FlatAdam
    from mopa_amd.pseudo import FlatEMA
    torch.manual_seed(0)
    cfg = default_cfg()
    m2, m3 = build_model_2d(cfg)[0].cuda().train(), build_model_3d(cfg)[0].cuda().train()
    o2, o3 = FlatAdam(m2.parameters()), FlatAdam(m3.parameters())
    e2, e3 = FlatEMA(o2, 0.99), FlatEMA(o3, 0.99)
    b = synth.make_batch(scans)
    n = b["x"][0].shape[0]
    batch = {"ori_img": [t.cuda() for t in b["img"]], "ori_img_indices": [torch.from_numpy(i).cuda() for i in b["img_indices"]],
             "ori_x": [b["x"][0].cuda(), b["x"][1].cuda()], "gather": torch.arange(n, device="cuda")}
    batch["geometry_3d"] = m3.net_3d.geometry(batch["ori_x"][0])
    return m2, m3, e2, e3, batch


def leg_byhand(m2, m3, e2, e3, batch):
    from mopa_amd import pseudo, scanprep

    def run():
        with torch.no_grad():
            with e2.average_parameters():
                m2.eval()
                l2 = torch.cat([m2({"img": batch["ori_img"][i].unsqueeze(0), "img_indices": [batch["ori_img_indices"][i]]})["seg_logit"]
                                for i in range(len(batch["ori_img"]))])
            with e3.average_parameters():
                m3.eval()
                l3 = m3({"x": batch["ori_x"], "geometry_3d": batch["geometry_3d"]})["seg_logit"]
            ps2, ps3 = pseudo.pseudo_labels(l2, l3, True)
            out = scanprep.take(batch, ps2), scanprep.take(batch, ps3)
        m2.train()
        m3.train()
        return out
    return run


def leg_teacher(m2, m3, e2, e3, batch, **kw):
    from mopa_amd.teacher import Teacher
    batched = kw.pop("batched", True)
    t = Teacher(m2, m3, e2, e3, **kw)
    return lambda: t.pseudo_labels(batch, True, batched=batched)


def measure(run, e2, e3, iters, warmup):
    host, dev, reserved = [], [], []
    for it in range(warmup + iters):
        e2.update()
        e3.update()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        run()
        t1 = time.perf_counter()
        b.record()
        torch.cuda.synchronize()
        if it < 3:   # (call 1 is the eager pass, call 2 records: the growth between them is the recorded key's private pool)
            reserved.append(round(torch.cuda.memory_reserved() / 2 ** 20, 1))
        if it >= warmup:
            host.append((t1 - t0) * 1e3)
            dev.append(a.elapsed_time(b))
    return {"host_ms_median": round(statistics.median(host), 3), "host_ms_min": round(min(host), 3),
            "device_ms_median": round(statistics.median(dev), 3), "device_ms_min": round(min(dev), 3), "iters": iters,
            "reserved_MB_after_calls_1_2_3": reserved}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="byhand,eager,replay,perimg")
    ap.add_argument("--scans", default="8,1")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        commit = "unknown"
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "results": {}}
    for scans in [int(s) for s in args.scans.split(",")]:
        for leg in args.legs.split(","):
            m2, m3, e2, e3, batch = build(scans)
            if leg == "byhand":
                run = leg_byhand(m2, m3, e2, e3, batch)
            else:
                run = leg_teacher(m2, m3, e2, e3, batch, **{"eager": dict(replay=False), "replay": {}, "perimg": dict(batched=False)}[leg])
            r = measure(run, e2, e3, args.iters, args.warmup)
            res["results"][f"{leg}@{scans}"] = r
            print(f"{leg:8s} scans={scans}: host {r['host_ms_median']:8.3f} ms  device {r['device_ms_median']:8.3f} ms", flush=True)
            del m2, m3, e2, e3, batch, run
            torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
