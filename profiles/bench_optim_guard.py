#!/usr/bin/env python3
"""What FlatAdam's gradient guard costs: device time of step() plain (one mopa_adam_flat launch) against guarded (mopa_grad_stats'
two launches + mopa_adam_flat_guarded), and of grad_stats() alone, over the parameter lists of the two networks (2D: 23.6 M
floats, 3D: 2.7 M).  One process, the legs alternating round by round, device events around `--batch` consecutive calls, after a
warm-up; medians and minima per call.

    python profiles/bench_optim_guard.py [--rounds 40] [--batch 10] [--warmup 5] [--out FILE.json]

The expectation from bytes: the update moves 28 B per element (p, g, m, v read; p, m, v written), the statistics pass reads 4 B
more -- one seventh -- plus two small launches.  Back-to-back steps find the 3D buffers (43 MB) in the Infinity Cache; in a
training iteration a whole forward + backward pass lies between two steps."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402


def build(which):
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d, build_model_3d
    from mopa_amd.optim import FlatAdam
    cfg = default_cfg()
    make = build_model_2d if which == "2d" else build_model_3d
    opts = []
    for kw in ({}, dict(max_grad_norm=1e9, skip_nonfinite=True)):     # nothing triggers: both take the same steps
        torch.manual_seed(0)
        model = make(cfg)[0].cuda().train()
        opts.append(FlatAdam(model.parameters(), lr=1e-3, **kw))
    g = torch.randn(opts[0].n, device="cuda") * 1e-3
    for o in opts:
        o.grad.copy_(g)
    return opts


def timed(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / batch       # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "batch": args.batch, "results": {}}
    for which in ("2d", "3d"):
        plain, guarded = build(which)
        legs = {"plain_step": plain.step, "guarded_step": guarded.step, "grad_stats": guarded.grad_stats}
        times = {k: [] for k in legs}
        for r in range(args.warmup + args.rounds):
            for k, fn in legs.items():
                t = timed(fn, args.batch)
                if r >= args.warmup:
                    times[k].append(t)
        assert torch.equal(plain.flat, guarded.flat), "the guarded optimizer left the plain one's trajectory"
        st = guarded.last_stats
        out = {"floats": plain.n, "parameters": len(plain.params), "chunks": guarded._gs["n_chunks"],
               "grad_norm": float(st.norm), "n_skipped": int(st.n_skipped), "n_clipped": int(st.n_clipped)}
        for k, v in times.items():
            out[k + "_us_median"], out[k + "_us_min"] = round(statistics.median(v), 2), round(min(v), 2)
        out["guarded_over_plain_median"] = round(out["guarded_step_us_median"] / out["plain_step_us_median"], 3)
        out["plain_GBps"] = round(28.0 * plain.n / out["plain_step_us_median"] / 1e3, 1)
        out["grad_stats_GBps"] = round(4.0 * plain.n / out["grad_stats_us_median"] / 1e3, 1)
        res["results"][which] = out
        print(f"{which}: {plain.n} floats, {len(plain.params)} parameters, {out['chunks']} chunks: plain {out['plain_step_us_median']:.1f} us, "
              f"guarded {out['guarded_step_us_median']:.1f} us (x{out['guarded_over_plain_median']:.3f}), "
              f"grad_stats alone {out['grad_stats_us_median']:.1f} us", flush=True)
        del plain, guarded, legs
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
