#!/usr/bin/env python3
"""The parity-class operators of the image branch at the bench shape (16 images, stem grid 304 x 480), one launch per class
(dense2d.CONV_CLASSES = False) against one launch per pass (True), both from this build:
  the four decoder up-convolutions ConvTranspose2d(k2, s2): forward (into the right half of the join buffer) and weight gradient,
  the three stride-2 3x3 convolutions layer2-4.0.conv1: backward-data as the first writer of dx.
Prints us per call (HIP events around `reps` back-to-back calls) and checks that both forms leave the same bits.
Usage: python profiles/bench_conv_classes.py [B=16] [H=304] [W=480] [reps=20]"""
import sys

import torch

sys.path.insert(0, ".")
from mopa_amd import dense2d                                    # noqa: E402
from mopa_amd.dense2d import ConvOp, ConvTOp, Img, new_img       # noqa: E402

B, H, W, reps = (int(a) for a in (sys.argv[1:] + ["16", "304", "480", "20"][len(sys.argv) - 1:]))
dev = torch.device("cuda", 0)
torch.manual_seed(0)


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


def both(fn, result):
    """-> (us per class-launch form, us one-launch form, same bits)"""
    us, bits = [], []
    for on in (False, True):
        dense2d.CONV_CLASSES = on
        result().fill_(0.5)
        fn()
        torch.cuda.synchronize()
        bits.append(result().clone())
        us.append(timed(fn))
    return us[0], us[1], torch.equal(bits[0], bits[1])


rows = []
# decoder stage, Cin, Cout, input grid = the stem grid / div
for stage, cin, cout, div in (("dec_t_conv_stage5", 512, 256, 16), ("dec_t_conv_stage4", 256, 128, 8), ("dec_t_conv_stage3", 128, 64, 4),
                              ("dec_t_conv_stage2", 64, 64, 2)):
    h, w = H // div, W // div
    op = ConvTOp(torch.randn(cin, cout, 2, 2, device=dev) * 0.05, torch.randn(cout, device=dev))
    x = Img(torch.randn(B * h * w, cin, device=dev), B, h, w)
    join = torch.zeros(B * 4 * h * w, 2 * cout, device=dev)
    out = Img(join, B, 2 * h, 2 * w, cout, cout)
    flop = 2.0 * B * h * w * 4 * cin * cout
    rows.append((f"{stage} forward {cin}->{cout} @ {h}x{w}", flop) + both(lambda: op.forward(x, out), lambda: join))
    dout = Img(torch.randn(B * 4 * h * w, 2 * cout, device=dev), B, 2 * h, 2 * w, cout, cout)
    dw = torch.empty_like(op.w)
    rows.append((f"{stage} weight gradient", flop) + both(lambda: op.wgrad(x, dout, dw), lambda: dw))
    del x, join, out, dout
for layer, cin, cout, div in (("layer2.0.conv1", 64, 128, 2), ("layer3.0.conv1", 128, 256, 4), ("layer4.0.conv1", 256, 512, 8)):
    h, w = H // div, W // div
    op = ConvOp(torch.randn(cout, cin, 3, 3, device=dev) * 0.05, None, 3, 2, 1)
    oh, ow = op.out_hw(h, w)
    x = Img(torch.empty(B * h * w, cin, device=dev), B, h, w)
    dout = Img(torch.randn(B * oh * ow, cout, device=dev), B, oh, ow)
    dx = new_img(B, h, w, cin, dev)
    wt = dense2d.relayout_cached(op.w, (3, 3, cout, cin), cout, cin, 3, 3, 1)
    flop = 2.0 * B * oh * ow * 9 * cin * cout
    rows.append((f"{layer} backward-data {cout}->{cin} @ {h}x{w}, first writer", flop) +
                both(lambda: op.dgrad_s2(x, dout, dx, wt, False), lambda: dx.t))
    rows.append((f"{layer} backward-data, accumulating", flop) + both(lambda: op.dgrad_s2(x, dout, dx, wt, True), lambda: dx.t))
print(f"{B} images, stem grid {H} x {W}; us per call over {reps} back-to-back calls")
print(f"{'operator':72s} {'per class':>10s} {'one launch':>10s} {'ratio':>6s} {'TF/s':>13s}  same bits")
for name, flop, a, b, same in rows:
    print(f"{name:72s} {a:10.1f} {b:10.1f} {a / b:6.2f} {flop / a / 1e6:6.1f}->{flop / b / 1e6:5.1f}  {same}")
print(f"sum: {sum(r[2] for r in rows):.1f} -> {sum(r[3] for r in rows):.1f} us")
assert all(r[4] for r in rows)
