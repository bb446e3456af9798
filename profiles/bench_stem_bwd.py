#!/usr/bin/env python3
"""The image branch's backward tail at the bench shape (16 images of 302 x 480 -> stem grid 16 x 304 x 480, two BatchNorm groups), the
first form against the second (dense2d.STEM_BWD2), per launch and as a chain, both from this build:
  first:  mopa_maxpool3x3s2_bwd (accumulating into the 64-channel half of the 128-wide join gradient), mopa_bn_bwd_sums_groups,
          mopa_stem_bwd_weight_bn (k_stem_wgrad_mfma + k_reduce_slabs2), mopa_conv2d_stem_relayout
  second: mopa_bn_bwd_sums_groups_pool, mopa_stem_bwd_weight_bn2 (k_stem_wgrad_strip + k_reduce_slabs_stem)
Prints us per call (HIP events around `reps` back-to-back calls), the matrix-pipe fraction of the weight gradient and checks that both
chains leave the same bits.  Usage: python profiles/bench_stem_bwd.py [B=16] [H=304] [W=480] [G=2] [reps=20]"""
import ctypes
import sys

import torch

sys.path.insert(0, ".")
from mopa_amd._lib import call, ptr, query, stream, workspace   # noqa: E402
from mopa_amd.dense2d import _geom                              # noqa: E402

B, H, W, G, reps = (int(a) for a in (sys.argv[1:] + ["16", "304", "480", "2", "20"][len(sys.argv) - 1:]))
dev = torch.device("cuda", 0)
torch.manual_seed(0)
rows, OH, OW = B * H * W, (H + 1) // 2, (W + 1) // 2
x4 = torch.randn(B, H + 6, W + 8, 4, device=dev)
J = torch.randn(rows, 128, device=dev)            # the raw stem output in the left half (the BatchNorm's input)
dJ0 = torch.randn(rows, 128, device=dev)          # the join gradient before the tail
stats = torch.empty(G, 4, 64, device=dev)
stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3] = 1.0, 0.1, 0.0, 1.0
pooled, amax = torch.empty(B * OH * OW, 64, device=dev), torch.empty(B * OH * OW * 64, dtype=torch.uint8, device=dev)
call("mopa_maxpool3x3s2_fwd_bn", ptr(J), 128, B, H, W, 64, ptr(stats), G, ptr(pooled), 64, ptr(amax), stream())
dpool = torch.randn(B * OH * OW, 64, device=dev)
geom = _geom(B=B, IH=H + 6, IW=W + 8, OHl=H, OWl=W, OHa=H, OWa=W, IDX=4, TH=7, TW=2, KWF=2, Cin=16, Cout=64, ld_in=4, ld_out=128)
wb = query("mopa_conv2d_wgrad_workspace_bytes", ctypes.addressof(geom))
bb = query("mopa_bnrelu_rows_workspace_bytes", rows, 64)
ws = workspace.get(max(wb, bb), dev)
n = rows // G


def chain(second, dJ, pg, coef, dw, dwl):
    steps = []
    if second:
        steps.append(("mopa_bn_bwd_sums_groups_pool", lambda: call(
            "mopa_bn_bwd_sums_groups_pool", ptr(dpool), 64, ptr(amax), B, H, W, ptr(dJ), 128, 1, ptr(J), 128, 64, G, ptr(stats), 0.0, 1,
            ptr(pg), ptr(pg, 64), 0, ptr(coef), ptr(ws), bb, stream())))
        steps.append(("mopa_stem_bwd_weight_bn2", lambda: call(
            "mopa_stem_bwd_weight_bn2", ptr(x4), ptr(dJ), 128, ptr(J), 128, ptr(stats), ptr(coef), G, 1, ptr(dw), ctypes.addressof(geom), 2,
            ptr(ws), wb, stream())))
    else:
        steps.append(("mopa_maxpool3x3s2_bwd", lambda: call(
            "mopa_maxpool3x3s2_bwd", ptr(dpool), 64, ptr(amax), B, H, W, 64, ptr(dJ), 128, 1, stream())))
        steps.append(("mopa_bn_bwd_sums_groups", lambda: call(
            "mopa_bn_bwd_sums_groups", ptr(dJ), 128, ptr(J), 128, rows, 64, G, n, 2 * n, ptr(stats), 0.0, 1, None, 0, ptr(pg), ptr(pg, 64), 0,
            ptr(coef), ptr(ws), bb, stream())))
        steps.append(("mopa_stem_bwd_weight_bn", lambda: call(
            "mopa_stem_bwd_weight_bn", ptr(x4), ptr(dJ), 128, ptr(J), 128, ptr(stats), ptr(coef), G, 1, ptr(dwl), ctypes.addressof(geom), 0,
            ptr(ws), wb, stream())))
        steps.append(("mopa_conv2d_stem_relayout", lambda: call("mopa_conv2d_stem_relayout", ptr(dwl), ptr(dw), 64, 1, 0, stream())))
    return steps


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


res, out = {}, {}
for second in (False, True):
    dJ, pg, coef = dJ0.clone(), torch.empty(2, 64, device=dev), torch.empty(G, 2, 64, device=dev)
    dw, dwl = torch.empty(64, 3, 7, 7, device=dev), torch.empty(7, 2, 16, 64, device=dev)
    steps = chain(second, dJ, pg, coef, dw, dwl)
    for _, fn in steps:   # one pass from the same start for the bit comparison
        fn()
    torch.cuda.synchronize()
    out[second] = [t.clone() for t in (dJ, pg, coef, dw)]
    # (timed calls accumulate into dJ again and again: the values drift, the work per call does not)
    res[second] = [(name, timed(fn)) for name, fn in steps] + [("chain", timed(lambda: [fn() for _, fn in steps]))]
same = all(torch.equal(a, b) for a, b in zip(out[False], out[True]))
flop = 2.0 * rows * 224 * 64
slabs = wb // (224 * 64 * 4)
for second in (False, True):
    print("second form:" if second else "first form:")
    for name, us in res[second]:
        extra = f"  ({flop / us / 1e6:.1f} TFLOP/s, {flop / us / 1e6 / 157.3:.2f} of the f32 matrix peak)" if "bwd_weight" in name else ""
        print(f"  {name:32s} {us:9.1f} us{extra}")
wg = [dict(res[s])[k] for s, k in ((False, "mopa_stem_bwd_weight_bn"), (True, "mopa_stem_bwd_weight_bn2"))]
print(f"{B} x {H} x {W}, G = {G}: M = {rows:,} pixels in {slabs} slabs; matrix-pipe floor {flop / 157.3e6:.0f} us; "
      f"weight gradient {wg[0]:.0f} -> {wg[1]:.0f} us ({wg[0] / wg[1]:.2f} x); chain {dict(res[False])['chain']:.0f} -> "
      f"{dict(res[True])['chain']:.0f} us; same bits: {same}")
assert same
