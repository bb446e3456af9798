#!/usr/bin/env python3
"""The stem's two matrix kernels at the bench shape (16 images of 302 x 480 -> stem grid 16 x 304 x 480, two BatchNorm groups), each
alone, from the build in the current directory:
  forward:          mopa_conv2d_igemm on the stem geometry (7 x 32 padded slots) against mopa_stem_fwd (147 taps), raw output into the
                    left half of the 128-wide join buffer; same bits
  weight gradient:  mopa_stem_bwd_weight_bn2 (k_stem_wgrad_strip + k_reduce_slabs_stem, parameter layout) and the chain in front of
                    it (mopa_bn_bwd_sums_groups_pool); a digest of the gradient, to compare two builds
A build without mopa_stem_fwd (the parent of round 28) prints the implicit GEMM alone: run this file from both trees in one job.
Prints us per call (HIP events around `reps` back-to-back calls) and TFLOP/s over the 147 taps' 2 * M * 147 * 64 FLOP.
(profiles/bench_stem.py is the 3D network's stem.)  Usage: python profiles/bench_stem2d.py [B=16] [H=304] [W=480] [G=2] [reps=20]"""
import ctypes
import hashlib
import sys

import torch

sys.path.insert(0, ".")
from mopa_amd._abi import SIGNATURES                           # noqa: E402
from mopa_amd._lib import call, ptr, query, stream, workspace   # noqa: E402
from mopa_amd.dense2d import _geom                              # noqa: E402

B, H, W, G, reps = (int(a) for a in (sys.argv[1:] + ["16", "304", "480", "2", "20"][len(sys.argv) - 1:]))
dev = torch.device("cuda", 0)
torch.manual_seed(0)
rows, OH, OW = B * H * W, (H + 1) // 2, (W + 1) // 2
img = torch.rand(B, 3, H - 2, W, device=dev)
x4 = torch.empty(B, H + 6, W + 8, 4, device=dev)
call("mopa_img_to_nhwc4", ptr(img), B, H - 2, W, H, W, ptr(x4), stream())
w = torch.randn(64, 3, 7, 7, device=dev) * 0.05
w1 = torch.empty(7, 2, 16, 64, device=dev)
call("mopa_conv2d_stem_relayout", ptr(w), ptr(w1), 64, 0, 0, stream())
geom = _geom(B=B, IH=H + 6, IW=W + 8, OHl=H, OWl=W, OHa=H, OWa=W, IDX=4, TH=7, TW=2, KWF=2, Cin=16, Cout=64, ld_in=4, ld_out=128)
flop = 2.0 * rows * 147 * 64


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


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def line(name, us, note=""):
    print(f"  {name:32s} {us:9.1f} us  ({flop / us / 1e6:6.1f} TFLOP/s over the real taps, {flop / us / 1e6 / 157.3:.2f} of the f32 matrix peak){note}")


print(f"{B} x {H} x {W}, G = {G}: M = {rows:,} pixels; matrix-pipe floor of 147 taps {flop / 157.3e6:.0f} us, of 224 slots "
      f"{flop * 224 / 147 / 157.3e6:.0f} us")
# ---- forward
print("forward:")
J = torch.full((rows, 128), -1.0, device=dev)
fwd = {"mopa_conv2d_igemm": lambda: call("mopa_conv2d_igemm", ptr(x4), ptr(w1), None, ptr(J), ctypes.addressof(geom), 0, stream())}
if "mopa_stem_fwd" in SIGNATURES:
    fwd["mopa_stem_fwd"] = lambda: call("mopa_stem_fwd", ptr(x4), ptr(w1), ptr(J), ctypes.addressof(geom), stream())
outs = {}
for name, fn in fwd.items():
    J.fill_(-1.0)
    us = timed(fn)
    outs[name] = digest(J)
    line(name, us, f"  digest {outs[name]}")
if len(outs) == 2:
    same = outs["mopa_conv2d_igemm"] == outs["mopa_stem_fwd"]
    print(f"  same bits: {same}")
    assert same
# ---- weight gradient: the raw stem output stays in J's left half (the BatchNorm's input)
print("weight gradient:")
stats = torch.empty(G, 4, 64, device=dev)
stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3] = 1.0, 0.1, 0.0, 1.0
pooled, amax = torch.empty(B * OH * OW, 64, device=dev), torch.empty(B * OH * OW * 64, dtype=torch.uint8, device=dev)
call("mopa_maxpool3x3s2_fwd_bn", ptr(J), 128, B, H, W, 64, ptr(stats), G, ptr(pooled), 64, ptr(amax), stream())
dpool = torch.randn(B * OH * OW, 64, device=dev)
dJ = torch.randn(rows, 128, device=dev)
wb = query("mopa_conv2d_wgrad_workspace_bytes", ctypes.addressof(geom))
bb = query("mopa_bnrelu_rows_workspace_bytes", rows, 64)
ws = workspace.get(max(wb, bb), dev)
pg, coef, dw = torch.empty(2, 64, device=dev), torch.empty(G, 2, 64, device=dev), torch.empty(64, 3, 7, 7, device=dev)
sums = lambda: call("mopa_bn_bwd_sums_groups_pool", ptr(dpool), 64, ptr(amax), B, H, W, ptr(dJ), 128, 1, ptr(J), 128, 64, G,   # noqa: E731
                    ptr(stats), 0.0, 1, ptr(pg), ptr(pg, 64), 0, ptr(coef), ptr(ws), bb, stream())
wgrad = lambda: call("mopa_stem_bwd_weight_bn2", ptr(x4), ptr(dJ), 128, ptr(J), 128, ptr(stats), ptr(coef), G, 1, ptr(dw),      # noqa: E731
                     ctypes.addressof(geom), 2, ptr(ws), wb, stream())
sums()
wgrad()
torch.cuda.synchronize()
print(f"  gradient digest {digest(dw)} (one pass from the same start: equal between two builds = same bits)")
us_w = timed(wgrad)   # (dJ does not change between these calls)
line("mopa_stem_bwd_weight_bn2", us_w, f"  {wb // (224 * 64 * 4)} slabs")
print(f"  {'mopa_bn_bwd_sums_groups_pool':32s} {timed(sums):9.1f} us")
print(f"  {'chain':32s} {timed(lambda: (sums(), wgrad())):9.1f} us")
