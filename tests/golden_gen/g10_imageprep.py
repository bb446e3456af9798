"""Generate tests/golden/g10_imageprep.npz and tests/golden/g10_imageprep_fullsize.json by RUNNING the real calls of the 2D input
pipeline on the host: Pillow's ``Image.resize(size, Image.BILINEAR)`` and ``ImageEnhance`` (which torchvision's PIL path of
``ColorJitter`` calls; from knowledge -- torchvision itself is not installed), ``scipy.ndimage.zoom(order=0)``, the reference's own
``refine_sam_mask`` (mopa/data/utils/refine_pseudo_labels.py, imported from the checkout) and the datasets' own index expressions
(mopa/data/nuscenes/nuscenes_dataloader.py:356-357,380,395; mopa/data/semantic_kitti/semantic_kitti_dataloader.py:571-580,598,610).

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixtures are what travels).
Usage, from the repo root:  python tests/golden_gen/g10_imageprep.py PATH_TO_MOPA_CHECKOUT

Cases (prefix in the .npz; ``*_n`` = number of cases, per case ``<prefix><k>_*``):
  r*  resize: 4:1 both axes, a non-integer ratio to an odd width, rows only, columns only.
  j*  jitter ("ImageEnhance, which torchvision's PIL path calls; from knowledge"): all six orders x three factor sets (below 1,
      above 1, exactly 1.0, the bounds 0.6 / 1.4) on a smooth image and on one whose blends hit both clip ends; one and two
      operations.
  t*  to tensor: flip x normalisation.
  m*  masks: the area threshold met exactly (one id at the threshold, one a pixel below), the out-of-range last row of a 4:1 zoom
      (88 -> 22), max_h positive / zero limit / negative limit / None, a crop window with flip on an unzoomed mask.
  i*  indices: the resize form and the crop form, float32 and float64, with and without flip.
  p*  the whole pipeline on two small nuScenes-form samples (112 x 80 -> 56 x 40): img, ori_img, mask, indices.
The .json holds position-weighted 64-bit checksums of every output of the three real shapes at B = 8 + 8 (see ``fullsize_inputs``
and ``checksum``, which tests/test_gpu_imageprep.py defines identically).
"""
import importlib.util
import json
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance
from scipy.ndimage import zoom

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "g10_imageprep.npz")
OUT_FULL = os.path.join(ROOT, "tests", "golden", "g10_imageprep_fullsize.json")
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def _load(ref):
    spec = importlib.util.spec_from_file_location("ref_refine", os.path.join(ref, "mopa", "data", "utils", "refine_pseudo_labels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.refine_sam_mask


# ---------------------------------------------------------------------------- shared with tests/test_gpu_imageprep.py
def checksum(a) -> int:
    """Position-weighted sum of the array's bytes modulo 2^64."""
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).astype(np.uint64)
    return int((b * np.arange(1, b.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def smooth_image(rng, H, W):
    """Smooth plus noise: 8 x 8 blocks of a random colour, +-20 of noise per value."""
    coarse = rng.integers(0, 256, (H // 8 + 1, W // 8 + 1, 3))
    img = np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:H, :W] + rng.integers(-20, 21, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def block_mask(rng, H, W, cell=32, ids=120):
    coarse = rng.integers(0, ids, (H // cell + 1, W // cell + 1))
    return np.repeat(np.repeat(coarse, cell, 0), cell, 1)[:H, :W].astype(np.uint8)


FULL = {"nuscenes": dict(W=1600, H=900, resize=(400, 225), crop=None, n=3000, seed=101),
        "a2d2": dict(W=1920, H=1208, resize=(480, 302), crop=None, n=3000, seed=102),
        "kitti": dict(W=1242, H=375, resize=None, crop=(480, 302), n=3000, seed=103)}


def fullsize_inputs(name, B=16):
    """The B raw samples of a real shape from numpy.random.Generator(PCG64(seed)): image, SAM mask, float32 points (rows in the
    lower part of the image, like lidar returns), and the sample's draws."""
    c = FULL[name]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    H, W = c["H"], c["W"]
    out = []
    for b in range(B):
        s = {"image": smooth_image(rng, H, W), "sam_mask": block_mask(rng, H, W)}
        rows = rng.random(c["n"]) * (H * 0.6 - 1) + H * 0.4
        cols = rng.random(c["n"]) * (W - 1)
        s["points_img"] = np.stack([rows, cols], 1).astype(np.float32)
        order = ORDERS[int(rng.integers(0, 6))]
        s["jitter"] = (order, tuple(float(np.float32(rng.uniform(0.6, 1.4))) for _ in order))
        s["flip"] = bool(rng.random() < 0.5)
        if c["crop"]:
            left = int(rng.random() * (W + 1 - c["crop"][0]))
            s["crop"] = (left, H - c["crop"][1], left + c["crop"][0], H)
        out.append(s)
    return out
# ----------------------------------------------------------------------------


def pil_jitter(img, order, factors):
    im = Image.fromarray(img)
    for op, f in zip(order, factors):
        enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op]
        im = enh(im).enhance(f)
    return im


def to_tensor(im, flip, norm):
    image = np.array(im, dtype=np.float32) / 255.
    if flip:
        image = np.ascontiguousarray(np.fliplr(image))
    if norm:
        mean, std = np.asarray(norm[0], dtype=np.float32), np.asarray(norm[1], dtype=np.float32)
        image = (image - mean) / std
    return np.ascontiguousarray(np.moveaxis(image, -1, 0))


def mask_case(refine, src, size, max_h, window, flip, thre=0.1):
    m = src
    if size is not None:                                       # nuscenes_dataloader.py:363-368 (both factors are 0.25 there)
        m = zoom(src, (size[1] / src.shape[0], size[0] / src.shape[1]), order=0)
        assert m.shape == (size[1], size[0])
    m = refine(np.ascontiguousarray(m), max_area_thre=thre, max_h=max_h)
    if window is not None:
        left, top, right, bottom = window
        m = m[top:bottom, left:right]
    if flip:
        m = np.ascontiguousarray(np.fliplr(m))
    return np.ascontiguousarray(m)


def idx_resize(points_img, src_size, resize, flip):
    """nuscenes_dataloader.py:356-357,378-380,395."""
    points_img = points_img.copy()
    points_img[:, 0] = float(resize[1]) / src_size[1] * np.floor(points_img[:, 0])
    points_img[:, 1] = float(resize[0]) / src_size[0] * np.floor(points_img[:, 1])
    row_min = int(np.min(points_img, axis=0)[0])
    ori = points_img.copy().astype(np.int64)
    img_indices = points_img.astype(np.int64)
    if flip:
        img_indices[:, 1] = resize[0] - 1 - img_indices[:, 1]
    return img_indices, ori, row_min


def idx_crop(points_img, window, flip):
    """semantic_kitti_dataloader.py:561,571-580,598,610."""
    left, top, right, bottom = window
    ori = points_img.copy().astype(np.int64)
    row_min = int(np.min(points_img, axis=0)[0])
    keep_idx = points_img[:, 0] >= top
    keep_idx = np.logical_and(keep_idx, points_img[:, 0] < bottom)
    keep_idx = np.logical_and(keep_idx, points_img[:, 1] >= left)
    keep_idx = np.logical_and(keep_idx, points_img[:, 1] < right)
    points_img = points_img[keep_idx]
    points_img[:, 0] -= top
    points_img[:, 1] -= left
    img_indices = points_img.astype(np.int64)
    if flip:
        img_indices[:, 1] = (right - left) - 1 - img_indices[:, 1]
    return img_indices, keep_idx, ori, row_min


def main(ref):
    refine = _load(ref)
    rng = np.random.Generator(np.random.PCG64(10))
    out = {}

    # ---- resize
    cases = [((64, 48), (16, 12)), ((101, 57), (37, 23)), ((80, 40), (80, 13)), ((80, 40), (25, 40))]
    out["r_n"] = np.int64(len(cases))
    for k, ((W, H), size) in enumerate(cases):
        img = smooth_image(rng, H, W)
        out[f"r{k}_in"], out[f"r{k}_size"] = img, np.asarray(size)
        out[f"r{k}_out"] = np.array(Image.fromarray(img).resize(size, Image.BILINEAR))

    # ---- jitter
    smooth = smooth_image(rng, 30, 40)
    extreme = smooth.copy()
    extreme[::3, ::2] = rng.choice([0, 255], extreme[::3, ::2].shape).astype(np.uint8)
    extreme[1::3, 1::2, 0] = 255
    extreme[1::3, 1::2, 1:] = 0
    out["j_img"] = np.stack([smooth, extreme])
    by_op = [(1.23, 0.71, 1.37), (0.6, 1.4, 1.0), (1.4, 0.6, 0.83)]          # factor of (brightness, contrast, saturation)
    jc = [(i, order, tuple(fs[o] for o in order)) for i in (0, 1) for order in ORDERS for fs in by_op]
    jc += [(1, (1,), (1.4,)), (1, (0,), (0.6,)), (0, (2,), (1.4,)), (1, (2, 1), (0.0, 1.0)), (0, (1, 0), (0.95, 1.05)), (1, (), ())]
    out["j_n"] = np.int64(len(jc))
    hit_lo = hit_hi = False
    for k, (i, order, fs) in enumerate(jc):
        res = np.array(pil_jitter(out["j_img"][i], order, fs))
        out[f"j{k}_img"], out[f"j{k}_order"], out[f"j{k}_factor"], out[f"j{k}_out"] = np.int64(i), np.asarray(order, np.int64), np.asarray(fs, np.float64), res
        hit_lo |= bool((res == 0).any() and i == 1)
        hit_hi |= bool((res == 255).any() and i == 1)
    assert hit_lo and hit_hi

    # ---- to tensor
    out["t_in"] = smooth_image(rng, 23, 37)
    out["t_norm"] = np.asarray(NORM, np.float64)
    for k, (flip, norm) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        out[f"t{k}_flip"], out[f"t{k}_normalise"] = np.bool_(flip), np.bool_(norm)
        out[f"t{k}_out"] = to_tensor(Image.fromarray(out["t_in"]), flip, NORM if norm else None)

    # ---- masks
    mc = []
    # threshold equality: zoomed 20 x 28 = 560 pixels, 0.1 * 560 = 56: id 5 covers exactly 56 (goes), id 6 covers 55 (stays)
    z = rng.integers(10, 40, (20, 28)).astype(np.uint8)
    z.reshape(-1)[:56] = 5
    z.reshape(-1)[56:111] = 6
    src = np.repeat(np.repeat(z, 4, 0), 4, 1)
    zz = zoom(src, (0.25, 0.25), order=0)
    assert np.array_equal(zz, z) and (zz == 5).sum() == 56 and (zz == 6).sum() == 55
    mc.append((src, (28, 20), None, None, False))
    # 4:1 zoom whose last row falls outside: 88 -> 22
    assert (22 - 1) * ((88 - 1) / (22 - 1)) > 88 - 1
    src88 = block_mask(rng, 88, 120, cell=8, ids=40)
    src88[-8:] = 200                                            # the rows the last zoomed row would read
    assert (zoom(src88, (0.25, 0.25), order=0)[-1] == 0).all()
    mc.append((src88, (30, 22), None, None, False))
    for max_h in (15, 22, 25, 0, 40):                           # limits 7, 0, -3 (all but the last three rows), 22 (all), -18
        mc.append((src88, (30, 22), max_h, None, max_h == 25))
    # unzoomed mask, crop window, flip (the SemanticKITTI form)
    src_k = block_mask(rng, 40, 100, cell=6, ids=60)
    mc.append((src_k, None, 40 - 13, (31, 12, 81, 40), True))
    mc.append((src_k, None, None, (0, 0, 50, 28), False))
    out["m_n"] = np.int64(len(mc))
    for k, (src, size, max_h, window, flip) in enumerate(mc):
        out[f"m{k}_in"] = src
        out[f"m{k}_size"] = np.asarray(size if size else (-1, -1))
        out[f"m{k}_max_h"] = np.int64(-999999 if max_h is None else max_h)
        out[f"m{k}_window"] = np.asarray(window if window else (-1, -1, -1, -1))
        out[f"m{k}_flip"] = np.bool_(flip)
        res = mask_case(refine, src, size, max_h, window, flip)
        assert res.dtype == np.int32
        out[f"m{k}_out"] = res
    assert (out["m0_out"] == 5).sum() == 0 and (out["m0_out"] == 6).sum() == 55

    # ---- indices
    ic = []
    for dt in (np.float32, np.float64):
        for flip in (False, True):
            p = np.stack([rng.random(500) * 899.99, rng.random(500) * 1599.99], 1).astype(dt)
            p[:7] = np.asarray([[899.99, 1599.99], [0, 0], [3.999, 4.0], [4.0, 3.999], [450.5, 800.5], [7.0, 1596.0], [896.0, 1.0]], dt)
            ic.append(("resize", p, (1600, 900), (400, 225), None, flip))
        for flip in (False, True):
            p = np.stack([rng.random(500) * 374.99, rng.random(500) * 1241.99], 1).astype(dt)
            p[:4] = np.asarray([[73.0, 333.0], [72.99, 400.0], [374.99, 812.99], [200.0, 813.0]], dt)
            ic.append(("crop", p, (1242, 375), None, (333, 73, 813, 375), flip))
    out["i_n"] = np.int64(len(ic))
    for k, (form, p, src_size, resize, window, flip) in enumerate(ic):
        out[f"i{k}_form"], out[f"i{k}_in"], out[f"i{k}_src_size"], out[f"i{k}_flip"] = np.str_(form), p, np.asarray(src_size), np.bool_(flip)
        if form == "resize":
            idx, ori, row_min = idx_resize(p, src_size, resize, flip)
            out[f"i{k}_size"] = np.asarray(resize)
        else:
            idx, keep, ori, row_min = idx_crop(p, window, flip)
            out[f"i{k}_window"], out[f"i{k}_keep"] = np.asarray(window), keep
        out[f"i{k}_out"], out[f"i{k}_ori"], out[f"i{k}_row_min"] = idx, ori, np.int64(row_min)

    # ---- the whole pipeline, small: two nuScenes-form samples 112 x 80 -> 56 x 40 (2:1), masks, points, jitter, one flipped
    out["p_size"], out["p_norm"] = np.asarray((56, 40)), np.asarray(NORM, np.float64)
    for b in range(2):
        img, mask = smooth_image(rng, 80, 112), block_mask(rng, 80, 112, cell=10, ids=30)
        pts = np.stack([rng.random(300) * 50 + 29.5, rng.random(300) * 111.9], 1).astype(np.float32)
        order, fs, flip = ORDERS[2 + 3 * b], (0.8, 1.3, 1.1), b == 1
        idx, ori_idx, row_min = idx_resize(pts, (112, 80), (56, 40), flip)
        im = Image.fromarray(img).resize((56, 40), Image.BILINEAR)
        out[f"p{b}_image"], out[f"p{b}_sam_mask"], out[f"p{b}_points"] = img, mask, pts
        out[f"p{b}_order"], out[f"p{b}_factor"], out[f"p{b}_flip"] = np.asarray(order), np.asarray(fs, np.float64), np.bool_(flip)
        out[f"p{b}_img"] = to_tensor(pil_jitter(np.array(im), order, fs), flip, NORM)
        out[f"p{b}_ori_img"] = np.moveaxis(np.array(im, dtype=np.float32) / 255., -1, 0)
        out[f"p{b}_mask"] = mask_case(refine, mask, (56, 40), im.size[1] - row_min, None, flip)
        out[f"p{b}_idx"], out[f"p{b}_ori_idx"] = idx, ori_idx

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")

    # ---- the three real shapes, B = 8 + 8, every output as a checksum
    full = {}
    for name, c in FULL.items():
        samples = fullsize_inputs(name)
        imgs, oris, masks, idxs, ori_idxs, keeps = [], [], [], [], [], []
        for s in samples:
            im = Image.fromarray(s["image"])
            pts = s["points_img"]
            if c["resize"]:
                idx, ori_idx, row_min = idx_resize(pts, (c["W"], c["H"]), c["resize"], s["flip"])
                im = im.resize(c["resize"], Image.BILINEAR)
                mask = mask_case(refine, s["sam_mask"], c["resize"], im.size[1] - row_min, None, s["flip"])
                ori_im = im
            else:
                idx, keep, ori_idx, row_min = idx_crop(pts, s["crop"], s["flip"])
                keeps.append(keep)
                ori_im = im
                mask = mask_case(refine, s["sam_mask"], None, c["H"] - row_min, s["crop"], s["flip"])
                im = im.crop(s["crop"])
            oris.append(np.moveaxis(np.array(ori_im, dtype=np.float32) / 255., -1, 0))
            imgs.append(to_tensor(pil_jitter(np.array(im), *s["jitter"]), s["flip"], NORM))
            masks.append(mask)
            idxs.append(idx)
            ori_idxs.append(ori_idx)
        full[name] = {"img": checksum(np.stack(imgs)), "ori_img": checksum(np.stack(oris)), "sam_mask": checksum(np.stack(masks)),
                      "img_indices": checksum(np.concatenate(idxs)), "ori_img_indices": checksum(np.concatenate(ori_idxs)),
                      "n_indices": int(sum(len(i) for i in idxs)), "n_ignored": int(sum((m == -100).sum() for m in masks))}
        if keeps:
            full[name]["keep"] = checksum(np.concatenate(keeps).astype(np.uint8))
    with open(OUT_FULL, "w") as f:
        json.dump(full, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT_FULL)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
