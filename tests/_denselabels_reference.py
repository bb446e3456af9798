"""Numpy restatement of the dense 2D pseudo labels (``mopa_amd.imageprep.prepare_dense_pslabels``), written from the contract and
not from the reference's text; the yardstick of tests/test_denselabels_host.py (against fixture G17, which the reference's own
``refine_sam_2Dlabels`` produced) and tests/test_gpu_denselabels.py (random inputs).

Per sample: probs (N,) float32, labels (N,) uint8, points (N, 2) float [row, col], mask (H, W) uint8.

1. row of a point: ``off = float32(1 - p) / float32(C - 1)`` everywhere, ``p`` at the raw label; ``conf`` = its maximum, ``label'``
   = the first index of the maximum.
2. per class of ``label'`` the lower median ``sorted[(n - 1) // 2]`` of ``conf``, capped at float32(0.9); ``conf < thresh`` makes
   a point unreliable: label -100, row zero.
3. the point goes to pixel (int(row), int(col)), truncated toward zero; the last point in array order wins a pixel.
4. every mask id with fewer than ``area_min_count`` pixels is filled with the first arg-max of the sum (float64 here) of its
   pixels' winning rows -- class 0 when all sums are zero; 5. the other pixels keep their winner's refined label, or -100.
6. crop window (left, top, right, bottom), then the left-right flip.

``decided()`` is the rule under which the float32 sums of the reference, the fixed-point sums of the device and the float64 sums
here must give one label: an id with k reliable winners is decided when ``s1 - s2 > 2 k 2^-23 s1`` for its two largest sums.
"""
import math

import numpy as np

IGNORE = -100


def area_min_count(max_area_thre, h, w):
    """Smallest pixel count of an id that is left alone: ``count >= max_area_thre * (h * w)`` evaluated in float32."""
    return int(math.ceil(float(np.float32(max_area_thre * (h * w)))))


def expand(probs, labels, C):
    """-> (conf float32, label' int64, off float32) of the never-built (N, C) rows."""
    p = np.asarray(probs, np.float32)
    raw = np.asarray(labels).astype(np.int64)
    off = ((np.float32(1.0) - p) / np.float32(C - 1)).astype(np.float32)
    conf = np.maximum(p, off)
    lab = np.where(p > off, raw, np.where(p < off, np.where(raw != 0, 0, 1), 0))
    return conf, lab, off


def refine(conf, lab):
    """Per class the lower median capped at 0.9; below it -> -100."""
    out = lab.copy()
    for c in np.unique(lab):
        sel = np.flatnonzero(lab == c)
        v = np.sort(conf[sel])
        thresh = min(v[(len(v) - 1) // 2], np.float32(0.9))
        out[sel[conf[sel] < thresh]] = IGNORE
    return out


def id_sums(probs, labels, points, mask, C):
    """-> (refined labels per point, winner map (H, W) of point indices or -1, {id: (area, k, float64 sums (C,))})."""
    H, W = mask.shape
    p = np.asarray(probs, np.float32)
    raw = np.asarray(labels).astype(np.int64)
    conf, lab, off = expand(p, raw, C)
    refined = refine(conf, lab) if len(p) else lab
    pts = np.asarray(points)
    rows, cols = np.trunc(pts[:, 0]).astype(np.int64), np.trunc(pts[:, 1]).astype(np.int64)
    assert ((rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)).all() and (raw < C).all()
    winner = np.full(H * W, -1, np.int64)
    winner[rows * W + cols] = np.arange(len(p))               # numpy assigns repeated indices in order: the last point stays
    win = winner[winner >= 0]
    win = win[refined[win] != IGNORE]                         # the reliable winners
    ids = mask.reshape(-1)[rows[win] * W + cols[win]].astype(np.int64)
    sums = np.zeros((256, C), np.float64)
    rows_w = np.repeat(off[win].astype(np.float64)[:, None], C, 1)
    rows_w[np.arange(len(win)), raw[win]] = p[win].astype(np.float64)
    np.add.at(sums, ids, rows_w)
    area, k = np.bincount(mask.reshape(-1), minlength=256), np.bincount(ids, minlength=256)
    stats = {int(mid): (int(area[mid]), int(k[mid]), sums[mid]) for mid in np.flatnonzero(area)}
    return refined, winner.reshape(H, W), stats


def decided(stats, min_count):
    """Ids below the area threshold whose label the sums do NOT decide (empty ids are decided: every sum is zero)."""
    bad = []
    for mid, (area, k, s) in stats.items():
        if area >= min_count or k == 0:
            continue
        top = np.sort(s)[::-1]
        if not top[0] - top[1] > 2 * k * 2.0 ** -23 * top[0]:
            bad.append(mid)
    return bad


def dense_pslabels(probs, labels, points, mask, C=10, max_area_thre=0.1, window=None, flip=False, return_undecided=False):
    """The (oh, ow) int32 label map of one sample."""
    H, W = mask.shape
    min_count = area_min_count(max_area_thre, H, W)
    refined, winner, stats = id_sums(probs, labels, points, mask, C)
    out = np.where(winner >= 0, refined[np.maximum(winner, 0)] if len(refined) else IGNORE, IGNORE).astype(np.int32)
    for mid, (area, k, s) in stats.items():
        if area < min_count:
            out[mask == mid] = int(np.argmax(s))              # numpy's argmax is the first maximum
    if window is not None:
        left, top, right, bottom = window
        out = out[top:bottom, left:right]
    if flip:
        out = out[:, ::-1]
    out = np.ascontiguousarray(out)
    return (out, decided(stats, min_count)) if return_undecided else out


# ---------------------------------------------------------------------------- inputs shared by the generator and the tests
def checksum(a) -> int:
    """Position-weighted sum of the array's bytes modulo 2^64 (as in G10)."""
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).astype(np.uint64)
    return int((b * np.arange(1, b.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def random_sample(rng, H, W, n, cell, ids, C=10, big_rows=0, patch=None):
    """One sample from a numpy Generator: a mask of ``cell`` x ``cell`` blocks with ids in [1, ids) (the rows ``[:big_rows]`` are
    id 0), n float32 points (all inside ``patch`` = (row0, col0, rows, cols) when given), raw labels that follow the block's id
    three times out of four -- so that the sums decide every id -- and probabilities in [0.35, 1) with one in sixteen at 0.05."""
    coarse = rng.integers(1, ids, (H // cell + 1, W // cell + 1))
    mask = np.repeat(np.repeat(coarse, cell, 0), cell, 1)[:H, :W].astype(np.uint8)
    mask[:big_rows] = 0
    r0, c0, nr, nc = patch if patch else (0, 0, H, W)
    pts = np.stack([r0 + rng.random(n) * (nr - 0.01), c0 + rng.random(n) * (nc - 0.01)], 1).astype(np.float32)
    at = mask[pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64)].astype(np.int64)
    labels = np.where(rng.random(n) < 0.75, (at * 7 + 3) % C, rng.integers(0, C, n)).astype(np.uint8)
    probs = (0.35 + 0.65 * rng.random(n)).astype(np.float32)
    probs[rng.random(n) < 1 / 16] = np.float32(0.05)
    return {"probs": probs, "labels": labels, "points": pts, "mask": mask}


FULL = dict(H=370, W=1226, n=20000, cell=32, ids=195, big_rows=111, B=8, seed=1700, crop=(480, 302))


def fullsize_inputs():
    """B = 8 samples at the SemanticKITTI shape (370 x 1226, 20,000 points, ids below 195 in 32-pixel blocks, id 0 large), with the
    draws of the cropped form: a 480 x 302 bottom crop and a flip per sample."""
    rng = np.random.Generator(np.random.PCG64(FULL["seed"]))
    out = []
    for b in range(FULL["B"]):
        s = random_sample(rng, FULL["H"], FULL["W"], FULL["n"], FULL["cell"], FULL["ids"], big_rows=FULL["big_rows"])
        left = int(rng.random() * (FULL["W"] + 1 - FULL["crop"][0]))
        s["window"] = (left, FULL["H"] - FULL["crop"][1], left + FULL["crop"][0], FULL["H"])
        s["flip"] = bool(rng.random() < 0.5)
        out.append(s)
    return out
