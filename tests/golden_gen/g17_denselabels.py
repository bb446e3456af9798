"""Generate tests/golden/g17_denselabels.npz and tests/golden/g17_denselabels_fullsize.json by RUNNING the reference's own
``refine_sam_2Dlabels`` (mopa/data/utils/refine_pseudo_labels.py, imported from the checkout) with ``torch.set_num_threads(1)``
behind the dataloader's row expansion (mopa/data/semantic_kitti/semantic_kitti_dataloader.py:445-449) and in front of the crop and
flip of ``__getitem__`` (:587-590, :611-613).

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixtures are what travels).
Usage, from the repo root:  python tests/golden_gen/g17_denselabels.py PATH_TO_MOPA_CHECKOUT

Cases of the .npz (``n`` = their number; per case ``c<k>_probs / labels / points / mask / window / flip / out``, window -1 = none):
  0     20 x 28 (threshold 56 pixels), made by hand: id 5 exactly at the threshold (left alone) and id 6 one pixel below (filled),
        id 0 small, an id without any point and two ids whose only points are unreliable (all three become 0), duplicate pixels
        (in a filled id and in the id that is left alone), a point with p = 0.05 (its label flips to 0), a class whose median is
        above 0.9 (the cap), a class with one point.
  1     24 x 40 with 8 x 8 blocks, id 0 large, random points.
  2     float64 points, 23 x 37.
  3..6  40 x 100 with crop windows at odd left origins and odd widths, with and without flip.
Every case is asserted to have no undecided id (tests/_denselabels_reference.py::decided), and the numpy restatement there is
asserted to equal the reference on every pixel.  The .json holds position-weighted checksums (``checksum``) of the B = 8 outputs at
370 x 1226 with 20,000 points each (``fullsize_inputs``), uncropped and with the samples' 480 x 302 crop + flip.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _denselabels_reference as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g17_denselabels.npz")
OUT_FULL = os.path.join(ROOT, "tests", "golden", "g17_denselabels_fullsize.json")


def _load(ref):
    spec = importlib.util.spec_from_file_location("ref_refine", os.path.join(ref, "mopa", "data", "utils", "refine_pseudo_labels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.refine_sam_2Dlabels


def reference(refine, s, window=None, flip=False):
    """semantic_kitti_dataloader.py:445-451, :587-590, :611-613 on one sample."""
    p, raw_ps_label_2d = s["probs"], s["labels"].astype(np.int32)
    probs_2d = np.zeros((p.shape[0], 10))
    probs_2d += np.expand_dims((1 - p) / 9, axis=1)
    probs_2d[np.arange(len(raw_ps_label_2d)), raw_ps_label_2d] = p
    full = refine(probs_2d, s["points"], s["mask"])
    assert full.dtype == np.int32
    if window is not None:
        left, top, right, bottom = window
        full = full[top:bottom, left:right]
    if flip:
        full = np.ascontiguousarray(np.fliplr(full))
    return np.ascontiguousarray(full)


def checked(refine, s, window=None, flip=False):
    """The reference's output, asserted decided and equal to the restatement."""
    out = reference(refine, s, window, flip)
    mine, undecided = R.dense_pslabels(s["probs"], s["labels"], s["points"], s["mask"], 10, 0.1, window, flip, return_undecided=True)
    assert not undecided, f"undecided ids {undecided}"
    assert np.array_equal(out, mine), "the restatement differs from the reference"
    return out


def hand_case():
    H, W = 20, 28
    m = np.zeros(H * W, np.int64)
    m[:56], m[56:111], m[111:123], m[123:140] = 5, 6, 0, 9
    m = m.reshape(H, W)
    for r in range(5, H):
        for c in range(W):
            m[r, c] = 10 + (r - 5) // 5 * 4 + c // 7           # ids 10..21, 35 pixels each
    pts, lab, pr = [], [], []

    def add(r, c, l, p):
        pts.append((r, c)); lab.append(l); pr.append(p)
    # id 5 (rows 0-1: exactly 56 pixels, left alone): two points, then a duplicate pixel whose LAST point is another class
    # (the 0.7 is below its class's median: its pixel holds -100)
    add(0.5, 3.2, 2, 0.8); add(1.1, 20.9, 2, 0.7); add(0.9, 3.9, 6, 0.85); add(1.5, 10.0, 2, 0.95)
    # id 6 (55 pixels, filled): class 3 with a median above 0.9 -- 0.91 is below the median 0.95 and stays (the cap)
    for k, p in enumerate((0.99, 0.97, 0.95, 0.93, 0.91)):
        add(2.0 + 0.1 * k, 2.0 + 3 * k, 3, p)
    add(2.2, 2.7, 1, 0.6)                                      # duplicate of (2, 2) in a filled id: the later, weaker row counts
    # id 0 small (12 pixels from (3, 27)): class 2
    add(4.0, 0.5, 2, 0.9); add(4.3, 5.0, 2, 0.75)
    # id 10: no point at all.  id 11: three points of class 5, all below that class's median.  id 12: one point, unreliable.
    for c in (8.0, 9.5, 12.0):
        add(6.0, c, 5, 0.2)
    add(7.0, 15.0, 5, 0.25)
    for c in (1.0, 2.0, 3.0, 4.0, 5.0):                        # the reliable half of class 5, in id 14
        add(11.0, c, 5, 0.6 + 0.05 * c)
    # id 13: p = 0.05 with raw label 4 -> off = 0.1056, label' 0; beside it the one point of class 7, a class-0 point and
    # p = 0.08 with raw label 0 -> label' 1
    add(6.5, 22.0, 4, 0.05); add(8.0, 23.0, 7, 0.5); add(9.0, 24.0, 0, 0.3); add(9.5, 25.0, 0, 0.08)
    # the rest: class 8 in ids 15..21
    for k in range(12):
        add(10.5 + 0.7 * k, 8.0 + 1.5 * k, 8, 0.5 + 0.03 * k)
    return {"probs": np.asarray(pr, np.float32), "labels": np.asarray(lab, np.uint8), "points": np.asarray(pts, np.float32),
            "mask": m.astype(np.uint8)}


def main(ref):
    torch.set_num_threads(1)
    refine = _load(ref)
    rng = np.random.Generator(np.random.PCG64(17))
    cases = []
    hand = hand_case()
    cases.append((hand, None, False))
    cases.append((R.random_sample(rng, 24, 40, 120, 8, 14, big_rows=5), None, False))
    s64 = R.random_sample(rng, 23, 37, 90, 6, 20)
    s64["points"] = s64["points"].astype(np.float64)
    cases.append((s64, None, True))
    sk = R.random_sample(rng, 40, 100, 400, 6, 60, big_rows=9)
    for window, flip in (((31, 12, 81, 40), True), ((33, 10, 80, 39), False), ((33, 10, 80, 39), True), ((0, 0, 50, 28), False)):
        cases.append((sk, window, flip))
    out = {"n": np.int64(len(cases))}
    for k, (s, window, flip) in enumerate(cases):
        for key in ("probs", "labels", "points", "mask"):
            out[f"c{k}_{key}"] = s[key]
        out[f"c{k}_window"] = np.asarray(window if window else (-1, -1, -1, -1))
        out[f"c{k}_flip"] = np.bool_(flip)
        out[f"c{k}_out"] = checked(refine, s, window, flip)

    # what the hand-made case is there for
    res, (refined, winner, stats) = out["c0_out"], R.id_sums(hand["probs"], hand["labels"], hand["points"], hand["mask"], 10)
    m = hand["mask"]
    assert stats[5][0] == 56 and stats[6][0] == 55 and R.area_min_count(0.1, 20, 28) == 56
    assert (res[m == 6] == 3).all() and (res[m == 0] == 2).all() and stats[0][0] == 12
    assert set(np.unique(res[m == 5])) == {-100, 2, 6} and res[0, 3] == 6               # left alone; the last point won (0, 3)
    assert stats[10][1] == 0 and not (winner[m == 10] >= 0).any() and (res[m == 10] == 0).all()
    for mid in (11, 12):
        assert stats[mid][1] == 0 and (winner[m == mid] >= 0).any() and (res[m == mid] == 0).all()
    conf, lab, off = R.expand(hand["probs"], hand["labels"], 10)
    i05 = int(np.flatnonzero(hand["probs"] == np.float32(0.05))[0])
    assert hand["labels"][i05] == 4 and lab[i05] == 0 and conf[i05] == off[i05]
    assert (refined[hand["labels"] == 3] == 3).all() and np.median(hand["probs"][hand["labels"] == 3]) > 0.9
    assert (lab == 7).sum() == 1 and refined[lab == 7][0] == 7
    assert len(hand["points"]) - (winner >= 0).sum() == 2 and res[1, 20] == -100                                # two duplicate pixels
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")

    samples = R.fullsize_inputs()
    plain = np.stack([checked(refine, s) for s in samples])
    crop = np.stack([checked(refine, s, s["window"], s["flip"]) for s in samples])
    full = {"plain": R.checksum(plain), "crop_flip": R.checksum(crop), "n_ignored_plain": int((plain == -100).sum()),
            "n_ignored_crop_flip": int((crop == -100).sum()), "shape_plain": list(plain.shape), "shape_crop_flip": list(crop.shape)}
    with open(OUT_FULL, "w") as f:
        json.dump(full, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT_FULL, full)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
