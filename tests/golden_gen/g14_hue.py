"""Generate tests/golden/g14_hue.npz by RUNNING Pillow: the hue step of torchvision's ``ColorJitter`` on a PIL image (``adjust_hue``:
``convert("HSV")``, ``np_h += np.int32(hue_factor * 255).astype(np.uint8)``, ``merge`` + ``convert("RGB")``; restated from
knowledge -- torchvision itself is not installed) alone and between ``ImageEnhance``'s three blends.

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixture is what travels).
Usage, from the repo root:  python tests/golden_gen/g14_hue.py

Refuses to write unless the numpy restatement of tests/_hue_reference.py equals Pillow on everything the fixture holds: the GPU
test names the first differing colour with that restatement, and the width / flip / batch tests take it as their reference.

Contents:
  full_shifts, full_crc32, full_sum   per shift in SHIFTS: zlib.crc32 and the byte sum of adjust_hue's output on the 4096 x 4096
                                      image of all 2^24 colours (``_hue_reference.all_colours``).
  img0 (37 x 53, smooth), img1 (5 x 300: a row crosses the kernel's 256-pixel segment; values at both clip ends), img2 (1 x 1)
  c_n cases ``c<k>_img / _order / _factor / _out``: all 24 orders of the four operations on each image, four factor sets
      (blend factors below and above 1, hue factors of both signs and the bounds +-0.5) rotating over them.
  w_*   one case read through a crop window of img0 (hue in front of contrast: the mean is the window's, after the shift).
  f_*   one flipped case (the output mirrored left to right).
"""
import itertools
import os
import sys
import zlib

import numpy as np
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _hue_reference as ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g14_hue.npz")
SHIFTS = (0, 1, 25, 128, 231, 255)
# factor of operation 0, 1, 2, 3
FACTORS = [(0.7, 0.8, 0.6, -0.07), (1.3, 1.25, 1.4, 0.09), (0.9, 1.37, 0.71, 0.5), (1.2, 0.65, 1.1, -0.5)]


def pil_hue_shift(im, shift):
    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(shift)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def pil_hue(im, factor):
    return pil_hue_shift(im, int(np.int32(factor * 255).astype(np.uint8)))


def pil_jitter(img, order, factors):
    im = Image.fromarray(img)
    for op, f in zip(order, factors):
        if op == ref.HUE:
            im = pil_hue(im, f)
        else:
            im = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](im).enhance(f)
    return np.asarray(im)


def checked(img, order, factors):
    want = pil_jitter(img, order, factors)
    got = ref.color_jitter(img, order, factors)
    if not np.array_equal(want, got):
        raise SystemExit(f"the restatement differs from Pillow for order {order}, factors {factors}: nothing written")
    return want


def images():
    rng = np.random.Generator(np.random.PCG64(14))
    coarse = rng.integers(0, 256, (37 // 8 + 1, 53 // 8 + 1, 3))
    img0 = np.clip(np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:37, :53] + rng.integers(-20, 21, (37, 53, 3)), 0, 255).astype(np.uint8)
    img1 = rng.integers(0, 256, (5, 300, 3)).astype(np.uint8)
    img1[:, ::7] = rng.choice(np.asarray([0, 255], np.uint8), (5, 43, 3))           # colours at the corners of the cube
    img1[2, 250:262] = np.arange(100, 112, dtype=np.uint8)[:, None]                 # greys (S = 0) across the segment boundary
    img2 = np.asarray([[[200, 30, 90]]], np.uint8)
    return [img0, img1, img2]


def main():
    d = {}
    allc = ref.all_colours()
    pil_all = Image.fromarray(allc)
    crc, tot = [], []
    for s in SHIFTS:
        want = np.asarray(pil_hue_shift(pil_all, s))
        if not np.array_equal(want, ref.adjust_hue_shift(allc, s)):
            raise SystemExit(f"the restatement differs from Pillow over all colours at shift {s}: nothing written")
        crc.append(zlib.crc32(want.tobytes()))
        tot.append(int(want.sum(dtype=np.uint64)))
    d["full_shifts"], d["full_crc32"], d["full_sum"] = np.asarray(SHIFTS, np.int32), np.asarray(crc, np.uint64), np.asarray(tot, np.uint64)
    for f, want in ((-0.5, 129), (-0.1, 231), (0.0, 0), (0.1, 25), (0.5, 127)):
        assert ref.hue_shift(f) == want == int(np.int32(float(np.float32(f)) * 255).astype(np.uint8)), f

    imgs = images()
    for i, im in enumerate(imgs):
        d[f"img{i}"] = im
    k = 0
    for i, im in enumerate(imgs):
        for n, order in enumerate(itertools.permutations(range(4))):
            fs = FACTORS[(n + i) % 4]
            factors = tuple(float(np.float32(fs[op])) for op in order)
            d[f"c{k}_img"], d[f"c{k}_order"] = np.int32(i), np.asarray(order, np.int32)
            d[f"c{k}_factor"], d[f"c{k}_out"] = np.asarray(factors, np.float64), checked(im, order, factors)
            k += 1
    d["c_n"] = np.int32(k)
    # read through a crop window (left, top, right, bottom)
    win, order = (5, 3, 45, 30), (3, 1, 0, 2)
    factors = tuple(float(np.float32(FACTORS[1][op])) for op in order)
    d["w_window"], d["w_order"], d["w_factor"] = np.asarray(win, np.int32), np.asarray(order, np.int32), np.asarray(factors, np.float64)
    d["w_out"] = checked(np.ascontiguousarray(imgs[0][win[1]:win[3], win[0]:win[2]]), order, factors)
    # flipped
    order = (2, 3, 1, 0)
    factors = tuple(float(np.float32(FACTORS[0][op])) for op in order)
    d["f_order"], d["f_factor"] = np.asarray(order, np.int32), np.asarray(factors, np.float64)
    d["f_out"] = np.ascontiguousarray(np.fliplr(checked(imgs[1], order, factors)))
    np.savez_compressed(OUT, **d)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", k, "cases")


if __name__ == "__main__":
    main()
