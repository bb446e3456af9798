"""Generate tests/golden/g11_scanprep.npz and tests/golden/g11_scanprep_fullsize.json by RUNNING the reference's 3D input
pipeline on the host: ``augment_and_scale_3d`` (mopa/data/utils/augmentation_3d.py), ``refine_pseudo_labels``
(mopa/data/utils/refine_pseudo_labels.py) and ``collate_scn_base`` (mopa/data/collate.py; its ``torchsparse.utils.collate`` import
is stubbed as oracle/gen_golden.py does), all imported from the checkout, plus the datasets' own expressions around them
(mopa/data/nuscenes/nuscenes_dataloader.py:339-340,410-465; mopa/data/semantic_kitti/semantic_kitti_dataloader.py:583-585,632-676).

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixtures are what travels).
Usage, from the repo root:  python tests/golden_gen/g11_scanprep.py PATH_TO_MOPA_CHECKOUT

The .npz holds ``meta`` (JSON: one entry per case -- name, B, scale, full_scale, the augmentation options and the seed each
sample's draws were made under, ema_input, refine) and per case ``k`` / sample ``b`` the inputs ``c<k>_s<b>_{points, seg_raw, img,
keep_in, pl2d, pr2d, pl3d, pr3d, teacher}``, the reference's draws ``_rot`` / ``_u`` / ``_next`` (the next ``np.random.rand()``
after the reference returned) and rotated points ``_aug_full``, and the outputs: ``c<k>_{locs, seg_label, ps2, ps3, ori_locs,
taken}`` (``collate_scn_base``'s ``x[0]``, ``seg_label``, ``pseudo_label_2d/3d``, ``ori_x[0]``; ``taken`` = the teacher labels
after the training loop's per-scan ``[ori_keep_idx][ori_idxs]``) and the lists ``c<k>_s<b>_{img_out, aug_out, orig_seg, idxs,
ori_ps3, ori_keep}``.  Cases: see ``small_cases``.  The .json holds position-weighted 64-bit checksums of every output of two
real shapes at B = 8 + 8 (``fullsize_inputs`` and ``checksum``, which tests/test_gpu_scanprep.py defines identically); those use
flips and the translation only: a +-1 diagonal makes ``points @ rot`` exact in any BLAS.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "g11_scanprep.npz")
OUT_FULL = os.path.join(ROOT, "tests", "golden", "g11_scanprep_fullsize.json")


def _load(ref):
    def mod(name, *path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *path))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    tsc = types.ModuleType("torchsparse.utils.collate")
    tsc.sparse_collate = lambda *a, **k: None
    sys.modules.update({"torchsparse": types.ModuleType("torchsparse"), "torchsparse.utils": types.ModuleType("torchsparse.utils"),
                        "torchsparse.utils.collate": tsc})
    aug = mod("ref_aug3d", "mopa", "data", "utils", "augmentation_3d.py").augment_and_scale_3d
    refine = mod("ref_refine", "mopa", "data", "utils", "refine_pseudo_labels.py").refine_pseudo_labels
    collate = mod("ref_collate", "mopa", "data", "collate.py").collate_scn_base
    return aug, refine, collate


# ---------------------------------------------------------------------------- shared with tests/test_gpu_scanprep.py
def checksum(a) -> int:
    """Position-weighted sum of the array's bytes modulo 2^64."""
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).astype(np.uint64)
    return int((b * np.arange(1, b.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


FULL = {"nuscenes": dict(n=34880, keep_in=False, seed=111), "kitti": dict(n=120000, keep_in=True, seed=112)}
FULL_AUG = dict(noisy_rot=0.0, flip_x=0.5, flip_y=0.5, rot_z=0.0, transl=True)
FULL_CLASSES = 11


def fullsize_inputs(name, B=16):
    """The B raw samples of a real shape from numpy.random.Generator(PCG64(seed)): a 20 m x 20 m x 1.5 m cloud (every second sample
    with 11 points far above the cloud, which the field filter drops), raw uint8 labels, image indices, int32 pseudo labels
    with float32 probabilities, for the cropped form a keep mask; ``draw_seed``: the sample's draws are made under it."""
    c = FULL[name]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    n = c["n"]
    out = []
    for b in range(B):
        q = (rng.standard_normal((n, 3)) * np.array([20.0, 20.0, 1.5])).astype(np.float32)
        if b % 2:
            q[:11, 2] = np.abs(q[:11, 2]) * 40 + 250      # far above: dropped whatever the flips are
        s = {"points": q, "seg_raw": rng.integers(0, 40, n).astype(np.uint8),
             "img": np.stack([rng.integers(0, 225, n), rng.integers(0, 400, n)], 1).astype(np.int64),
             "pl2d": rng.integers(0, FULL_CLASSES, n).astype(np.int32), "pr2d": rng.random(n, dtype=np.float32),
             "pl3d": rng.integers(0, FULL_CLASSES, n).astype(np.int32), "pr3d": rng.random(n, dtype=np.float32) ** 0.25,
             "draw_seed": 1000 * c["seed"] + b}
        if c["keep_in"]:
            s["keep_in"] = rng.random(n) < 0.25
        out.append(s)
    mapping = rng.integers(0, FULL_CLASSES, 40).astype(np.int64)
    mapping[::7] = -100
    return out, mapping
# ---------------------------------------------------------------------------- end of the shared part


def cloud(rng, n, spread=(12.0, 12.0, 1.5)):
    return (rng.standard_normal((n, 3)) * np.array(spread)).astype(np.float32)


def side_arrays(rng, n, classes=6, absent=None):
    pl = rng.integers(0, classes, n)
    if absent is not None:
        pl[pl == absent] = (absent + 1) % classes
    s = {"seg_raw": rng.integers(0, 20, n).astype(np.int16), "img": np.stack([rng.integers(0, 40, n), rng.integers(0, 56, n)], 1).astype(np.int64),
         "pl2d": pl.astype(np.int64), "pr2d": rng.random(n, dtype=np.float32) ** 0.2,
         "pl3d": rng.integers(0, classes, n).astype(np.int64), "pr3d": rng.random(n, dtype=np.float32),
         "teacher": rng.integers(0, classes, n).astype(np.int64)}
    return s


def small_cases():
    """-> list of (meta, samples, mapping).  No augmentation; each option alone and all together, without and with translation; a
    partial drop (far points on the positive side) and far points on both sides; the cropped form (keep_in, one scan all false)
    with a label mapping that has -100 entries, pseudo labels and ema_input; pseudo labels with a class absent from one scan, an
    even and an odd class count and probabilities above 0.9; a 4-sample batch with everything."""
    rng = np.random.Generator(np.random.PCG64(11))
    mapping = rng.integers(0, 6, 20).astype(np.int64)
    mapping[[3, 11, 19]] = -100
    cases = []
    none = dict(noisy_rot=0.0, flip_x=0.0, flip_y=0.0, rot_z=0.0)

    def add(name, samples, aug, transl, ema=False, mapped=False, seed0=0):
        meta = dict(name=name, B=len(samples), scale=20, full_scale=4096, aug=dict(aug, transl=bool(transl)), ema_input=ema, refine=True,
                    seeds=[seed0 + b for b in range(len(samples))])
        cases.append((meta, samples, mapping if mapped else None))

    add("plain", [dict(points=cloud(rng, 300), **side_arrays(rng, 300)), dict(points=cloud(rng, 257), **side_arrays(rng, 257))], none, False)
    opts = [dict(none, noisy_rot=0.1), dict(none, flip_x=0.5), dict(none, flip_y=0.5), dict(none, rot_z=6.2831),
            dict(noisy_rot=0.1, flip_x=0.5, flip_y=0.5, rot_z=6.2831)]
    for transl in (False, True):
        for j, o in enumerate(opts):
            names = ["noisy_rot", "flip_x", "flip_y", "rot_z", "all"]
            add(names[j] + ("_transl" if transl else ""), [dict(points=cloud(rng, 150), **side_arrays(rng, 150)),
                                                             dict(points=cloud(rng, 130), **side_arrays(rng, 130))], o, transl, seed0=10 * j + 3)
    q = cloud(rng, 700)
    q[:11] = np.abs(q[:11]) * 40 + 50
    add("partial", [dict(points=q, **side_arrays(rng, 700)), dict(points=cloud(rng, 300), **side_arrays(rng, 300))], none, True, ema=True, seed0=70)
    q = cloud(rng, 700)
    q[:11] = q[:11] * 40 + np.sign(q[:11]) * 50
    add("both_sides", [dict(points=q, **side_arrays(rng, 700))], none, False, seed0=80)
    ks = []
    for b, n in enumerate((500, 400, 300)):
        s = dict(points=cloud(rng, n), **side_arrays(rng, n))
        s["keep_in"] = (rng.random(n) < 0.4) if b != 1 else np.zeros(n, bool)
        if b == 2:
            s["points"][:7, 2] = np.abs(s["points"][:7, 2]) * 40 + 250
            s["keep_in"][:7] = True
        ks.append(s)
    add("keep_in", ks, dict(none, flip_y=0.5), True, ema=True, mapped=True, seed0=90)
    a, b = dict(points=cloud(rng, 601), **side_arrays(rng, 601, absent=2)), dict(points=cloud(rng, 400), **side_arrays(rng, 400))
    a["pl3d"][:] = np.where(np.arange(601) < 300, 0, 1)          # class 0: an even count, class 1: an odd count
    a["pr3d"][:5] = np.float32(0.95)
    b["pr2d"][:] = np.float32(0.97) + rng.random(400, dtype=np.float32) * np.float32(0.02)   # a median above 0.9
    add("pseudo", [a, b], none, False, ema=True, seed0=100)
    four = [dict(points=cloud(rng, n), **side_arrays(rng, n)) for n in (350, 300, 420, 280)]
    four[2]["points"][:9, 2] = np.abs(four[2]["points"][:9, 2]) * 40 + 250
    add("collate4", four, dict(none, flip_x=0.5), True, ema=True, mapped=True, seed0=110)
    return cases


def replay_draws(aug):
    """The draws augment_and_scale_3d makes, in its order (as fixture G4 records them)."""
    rot = None
    if aug["noisy_rot"] > 0 or aug["flip_x"] > 0 or aug["flip_y"] > 0 or aug["rot_z"] > 0:
        rot = np.eye(3, dtype=np.float32)
        if aug["noisy_rot"] > 0:
            rot += np.random.randn(3, 3) * aug["noisy_rot"]
        if aug["flip_x"] > 0:
            rot[0][0] *= np.random.randint(0, 2) * 2 - 1
        if aug["flip_y"] > 0:
            rot[1][1] *= np.random.randint(0, 2) * 2 - 1
        if aug["rot_z"] > 0:
            theta = np.random.rand() * aug["rot_z"]
            rot = rot.dot(np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]], dtype=np.float32))
    u = np.random.rand(3) if aug["transl"] else None
    return rot, u


def run_reference(ref, samples, mapping, aug, seeds, scale, full_scale, ema):
    """The datasets' __getitem__ expressions around the reference's functions for every sample, then collate_scn_base.
    -> (collated dict, per-sample records)."""
    augment, refine, collate = ref
    dicts, recs = [], []
    for s, seed in zip(samples, seeds):
        n = len(s["points"])
        seg = mapping[s["seg_raw"]] if mapping is not None else s["seg_raw"].astype(np.int64)
        keep_idx = s["keep_in"] if "keep_in" in s else np.ones(n, dtype=np.bool_)
        ps2 = refine(s["pr2d"], s["pl2d"].astype(np.int32))
        ps3 = refine(s["pr3d"], s["pl3d"].astype(np.int32))
        rec = {}
        np.random.seed(seed)
        rot, u = replay_draws(aug)
        rec["next"] = np.random.rand()
        rec["rot"], rec["u"] = rot, u
        if keep_idx.any():
            points, seg_k, img_k = s["points"][keep_idx], seg[keep_idx], s["img"][keep_idx]
            np.random.seed(seed)
            coords, points = augment(points, scale, full_scale, **aug)
            assert np.random.rand() == rec["next"]
            coords = coords.astype(np.int64)
            idxs = (coords.min(1) >= 0) * (coords.max(1) < full_scale)
        else:                                  # the reference raises on the empty minimum: such a scan contributes no rows
            points, seg_k, img_k = s["points"][:0], seg[:0], s["img"][:0]
            coords, idxs = np.zeros((0, 3), np.int64), np.zeros(0, np.bool_)
        rec["aug_full"] = points
        d = {"coords": coords[idxs], "aug_points": points[idxs], "seg_label": seg_k[idxs], "img_indices": img_k[idxs],
             "img": np.zeros((3, 2, 2), np.float32), "orig_seg_label": seg_k, "orig_points_idx": idxs,
             "pseudo_label_2d": ps2[keep_idx][idxs], "pseudo_label_3d": ps3[keep_idx][idxs], "ori_pseudo_label_3d": ps3}
        d["feats"] = np.ones([d["coords"].shape[0], 1], np.float32)
        if ema:
            ori_coords, _ = augment(s["points"], scale, full_scale)
            ori_idxs = (ori_coords.min(1) >= 0) * (ori_coords.max(1) < full_scale)
            d.update({"ori_img": np.zeros((3, 2, 2), np.float32), "ori_img_indices": s["img"], "ori_coords": ori_coords[ori_idxs],
                      "aug_keep_idx": keep_idx, "ori_idxs": idxs})
            d["ori_feats"] = np.ones([d["ori_coords"].shape[0], 1], np.float32)
        rec["taken"] = s["teacher"][keep_idx][idxs] if "teacher" in s else None
        rec["aug_keep_idx"] = keep_idx
        dicts.append(d)
        recs.append(rec)
    return collate(dicts, output_orig=True), recs


def outputs(col, recs, ema):
    """Every compared output as numpy arrays: (batch-level dict, per-sample dict of lists)."""
    top = {"locs": col["x"][0].numpy(), "seg_label": col["seg_label"].numpy(), "ps2": col["pseudo_label_2d"].numpy().astype(np.int64),
           "ps3": col["pseudo_label_3d"].numpy().astype(np.int64)}
    lists = {"img_out": col["img_indices"], "aug_out": col["aug_points_ls"], "orig_seg": col["orig_seg_label"], "idxs": col["orig_points_idx"],
             "ori_ps3": [np.asarray(a).astype(np.int64) for a in col["ori_pslabel_ls"]]}
    if ema:
        top["ori_locs"] = col["ori_x"][0].numpy().astype(np.int64)
        # collate_scn_base(output_orig=True) overwrites its own 'ori_keep_idx' list of the EMA input with the (here empty) list of
        # the output_orig branch (collate.py:245,259): the masks are taken from the datasets' 'aug_keep_idx' themselves
        lists["ori_keep"] = [r["aug_keep_idx"] for r in recs]
        assert all(np.array_equal(a, b) for a, b in zip(col["ori_idxs"], col["orig_points_idx"]))
    if recs[0]["taken"] is not None:
        top["taken"] = np.concatenate([r["taken"] for r in recs])
    return top, lists


def main():
    ref = _load(sys.argv[1])
    save, metas = {}, []
    for k, (meta, samples, mapping) in enumerate(small_cases()):
        col, recs = run_reference(ref, samples, mapping, meta["aug"], meta["seeds"], meta["scale"], meta["full_scale"], meta["ema_input"])
        top, lists = outputs(col, recs, meta["ema_input"])
        kept = [int(np.sum(i)) for i in lists["idxs"]]
        meta["kept"], meta["mapped"] = kept, mapping is not None
        if meta["name"] == "partial":
            assert 0 < kept[0] < len(samples[0]["points"]), kept
        if mapping is not None:
            save[f"c{k}_mapping"] = mapping
        for b, (s, r) in enumerate(zip(samples, recs)):
            for key, v in s.items():
                save[f"c{k}_s{b}_{key}"] = v
            for key in ("rot", "u"):
                if r[key] is not None:
                    save[f"c{k}_s{b}_{key}"] = r[key]
            save[f"c{k}_s{b}_next"] = np.float64(r["next"])
            save[f"c{k}_s{b}_aug_full"] = r["aug_full"]
            for key, ls in lists.items():
                save[f"c{k}_s{b}_{key}"] = np.asarray(ls[b])
        for key, v in top.items():
            save[f"c{k}_{key}"] = v
        metas.append(meta)
        print(k, meta["name"], "kept", kept, "of", [len(s["points"]) for s in samples])
    save["meta"] = np.asarray(json.dumps(metas))
    np.savez_compressed(OUT, **save)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")

    full = {}
    for name, c in FULL.items():
        samples, mapping = fullsize_inputs(name)
        for s in samples:
            s["teacher"] = s["pl3d"].astype(np.int64)
        col, recs = run_reference(ref, samples, mapping, FULL_AUG, [s["draw_seed"] for s in samples], 20, 4096, True)
        top, lists = outputs(col, recs, True)
        sums = {key: checksum(v) for key, v in top.items()}
        for key, ls in lists.items():
            sums[key] = checksum(np.concatenate([np.asarray(a).astype(np.uint8) if np.asarray(a).dtype == np.bool_ else np.asarray(a) for a in ls]))
        sums["kept"] = [int(np.sum(i)) for i in lists["idxs"]]
        full[name] = sums
        print(name, "kept", sums["kept"])
    with open(OUT_FULL, "w") as f:
        json.dump(full, f, indent=1, sort_keys=True)
    print("wrote", OUT_FULL)


if __name__ == "__main__":
    main()
