"""mopa_amd/scanprep.py on the device against fixture G11 (the reference's augment_and_scale_3d, refine_pseudo_labels and
collate_scn_base run on the host by tests/golden_gen/g11_scanprep.py) and against the per-scan path it replaces
(voxelize.rotate_points + voxelize_scan, pseudo.refine_pseudo_labels).  Every comparison is an equality unless said.  Reads only
committed fixtures."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROT_CASES = ("noisy_rot", "rot_z", "all")       # a float32 product against a BLAS: the rotation test's bound, not equality


# ---------------------------------------------------------------------------- defined identically in tests/golden_gen/g11_scanprep.py
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


@pytest.fixture(scope="module")
def g11():
    g = np.load(os.path.join(GOLDEN, "g11_scanprep.npz"))
    return g, json.loads(str(g["meta"]))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_sample(s, rot=None, u=None, points=None, pseudo=True):
    d = {"points": cu(s["points"] if points is None else points), "rot": rot, "transl_u": u, "seg_label": cu(s["seg_raw"]),
         "img_indices": cu(s["img"])}
    if "keep_in" in s:
        d["keep_in"] = cu(s["keep_in"])
    if pseudo:
        d.update({"pseudo_label_2d": cu(s["pl2d"]), "probs_2d": cu(s["pr2d"]), "pseudo_label_3d": cu(s["pl3d"]), "probs_3d": cu(s["pr3d"])})
    return d


def case_samples(g, k, m, from_rotated):
    out, raw = [], []
    for b in range(m["B"]):
        s = {key: g[f"c{k}_s{b}_{key}"] for key in ("points", "seg_raw", "img", "keep_in", "pl2d", "pr2d", "pl3d", "pr3d", "teacher", "rot", "u",
                                                    "aug_full") if f"c{k}_s{b}_{key}" in g.files}
        pts = None
        if from_rotated:                      # the reference's own rotated points stand in for the points (rows outside keep_in do not matter)
            pts = s["points"].copy()
            pts[s["keep_in"] if "keep_in" in s else slice(None)] = s["aug_full"]
        out.append(device_sample(s, None if from_rotated else s.get("rot"), s.get("u"), pts))
        raw.append(s)
    return out, raw


def np_(t):
    return t.cpu().numpy()


def batch_outputs(batch, teacher=None):
    from mopa_amd import scanprep as sp
    top = {"locs": np_(batch["x"][0]), "seg_label": np_(batch["seg_label"]), "ps2": np_(batch["pseudo_label_2d"]), "ps3": np_(batch["pseudo_label_3d"])}
    lists = {"img_out": batch["img_indices"], "aug_out": batch["aug_points_ls"], "orig_seg": batch["orig_seg_label"],
             "idxs": batch["orig_points_idx"], "ori_ps3": batch["ori_pslabel_ls"]}
    if "ori_x" in batch:
        top["ori_locs"] = np_(batch["ori_x"][0])
        lists["ori_keep"] = batch["ori_keep_idx"]
        assert all(torch.equal(a, b) for a, b in zip(batch["ori_idxs"], batch["orig_points_idx"]))
        assert batch["ori_x"][1].shape == (len(top["ori_locs"]), 1) and bool((batch["ori_x"][1] == 1).all())
    if teacher is not None:
        top["taken"] = np_(sp.take(batch, teacher))
    return top, {k: [np_(t) for t in v] for k, v in lists.items()}


def check_structure(batch, B):
    locs, feats = batch["x"]
    M = locs.shape[0]
    assert locs.dtype == torch.int64 and locs.shape == (M, 4) and feats.dtype == torch.float32 and feats.shape == (M, 1)
    assert bool((feats == 1).all())
    off = np_(batch["offsets"])
    assert batch["offsets"].dtype == torch.int64 and off.shape == (B + 1,) and off[0] == 0 and off[-1] == M
    assert [len(a) for a in batch["aug_points_ls"]] == list(np.diff(off))
    assert batch["gather"].dtype == torch.int64 and batch["gather"].shape == (M,)
    assert batch["n_outside"].dtype == torch.int32
    for b in range(B):
        assert bool((locs[off[b]:off[b + 1], 3] == b).all())


def run_case(g, k, m, from_rotated, **kw):
    from mopa_amd import scanprep as sp
    samples, raw = case_samples(g, k, m, from_rotated)
    mapping = cu(g[f"c{k}_mapping"]) if m["mapped"] else None
    batch = sp.prepare_batch_3d(samples, scale=m["scale"], full_scale=m["full_scale"], label_mapping=mapping, refine=True,
                                ema_input=m["ema_input"], **kw)
    check_structure(batch, m["B"])
    return batch, raw, samples


def test_small_cases_from_the_reference_rotated_points_equal_g11(g11):
    """Every returned key of every G11 case, computed from the reference's own rotated points (rot=None).  The cases that combine
    a rotation with ema_input are left to the next test: their un-augmented copy needs the points as loaded."""
    g, meta = g11
    ran = 0
    for k, m in enumerate(meta):
        has_rot = f"c{k}_s0_rot" in g.files
        if has_rot and m["ema_input"]:
            continue
        batch, raw, _ = run_case(g, k, m, from_rotated=True)
        top, lists = batch_outputs(batch, cu(np.concatenate([s["teacher"] for s in raw])))
        for key, v in top.items():
            ref = g[f"c{k}_{key}"]
            assert v.dtype == ref.dtype and np.array_equal(v, ref), (m["name"], key)
        for key, ls in lists.items():
            for b, v in enumerate(ls):
                ref = g[f"c{k}_s{b}_{key}"]
                assert v.dtype == ref.dtype and v.shape == ref.shape and np.array_equal(v, ref), (m["name"], key, b)
        ran += 1
    assert ran >= 14


def parent_path(raw_samples, draws, scale, full_scale):
    """rotate_points + voxelize_scan per scan: the path that exists without scanprep."""
    from mopa_amd.voxelize import rotate_points, voxelize_scan
    locs, keeps, augs = [], [], []
    for b, (s, (rot, u)) in enumerate(zip(raw_samples, draws)):
        pts = cu(s["points"])
        if "keep_in" in s:
            pts = pts[cu(s["keep_in"])]
        if pts.shape[0] == 0:
            locs.append(torch.zeros(0, 4, dtype=torch.int64, device="cuda"))
            keeps.append(torch.zeros(0, dtype=torch.bool, device="cuda"))
            augs.append(pts)
            continue
        c, keep = voxelize_scan(pts, scale, full_scale, u, b, rot=rot)
        locs.append(c)
        keeps.append(keep)
        augs.append(rotate_points(pts, rot)[keep])
    return torch.cat(locs), keeps, augs


def test_from_raw_points_equals_the_per_scan_path_and_g11_within_the_rotation_bound(g11):
    g, meta = g11
    for k, m in enumerate(meta):
        batch, raw, _ = run_case(g, k, m, from_rotated=False)
        locs, keeps, augs = parent_path(raw, [(s.get("rot"), s.get("u")) for s in raw], m["scale"], m["full_scale"])
        assert torch.equal(batch["x"][0], locs), m["name"]
        for b in range(m["B"]):
            assert torch.equal(batch["orig_points_idx"][b], keeps[b]), (m["name"], b)
            assert torch.equal(batch["aug_points_ls"][b], augs[b]), (m["name"], b)
        top, lists = batch_outputs(batch, cu(np.concatenate([s["teacher"] for s in raw])))
        exact = not m["name"].startswith(ROT_CASES)
        for key, v in top.items():
            ref = g[f"c{k}_{key}"]
            if exact or key != "locs":
                assert v.dtype == ref.dtype and np.array_equal(v, ref), (m["name"], key)
            else:          # the bound of test_device_rotation_stage_replays_the_reference_augmentation
                assert v.shape == ref.shape and np.abs(v - ref).max() <= 1, m["name"]
                assert (v == ref).all(1).mean() >= 0.99, m["name"]
        for key, ls in lists.items():
            for b, v in enumerate(ls):
                ref = g[f"c{k}_s{b}_{key}"]
                if exact or key != "aug_out":
                    assert v.dtype == ref.dtype and v.shape == ref.shape and np.array_equal(v, ref), (m["name"], key, b)
                else:
                    assert v.shape == ref.shape and np.abs(v - ref).max() <= 2 * np.spacing(np.abs(ref).max().astype(np.float32))


def test_full_size_batch_with_every_rotation_option_equals_the_per_scan_path():
    from mopa_amd import scanprep as sp
    raw, _ = fullsize_inputs("nuscenes")
    draws = []
    for s in raw:
        np.random.seed(s["draw_seed"])
        draws.append(sp.draw_augmentation_3d(noisy_rot=0.1, flip_x=0.5, flip_y=0.5, rot_z=6.2831, transl=True))
    samples = [device_sample(s, rot, u) for s, (rot, u) in zip(raw, draws)]
    batch = sp.prepare_batch_3d(samples, scale=20, full_scale=4096)
    check_structure(batch, 16)
    locs, keeps, augs = parent_path(raw, draws, 20, 4096)
    assert torch.equal(batch["x"][0], locs)
    assert all(torch.equal(a, b) for a, b in zip(batch["orig_points_idx"], keeps))
    assert all(torch.equal(a, b) for a, b in zip(batch["aug_points_ls"], augs))
    kept = [int(k.sum()) for k in keeps]
    assert 0 < min(kept) and any(k < 34880 for k in kept)
    flat = torch.cat(keeps).nonzero().squeeze(1)
    assert torch.equal(batch["gather"], flat)
    assert torch.equal(batch["seg_label"], torch.cat([d["seg_label"] for d in samples]).long()[flat])
    assert all(torch.equal(a, d["img_indices"][k]) for a, d, k in zip(batch["img_indices"], samples, keeps))


def test_segmented_refinement_equals_one_call_per_scan_and_array():
    from mopa_amd import scanprep as sp
    from mopa_amd.pseudo import refine_pseudo_labels
    raw, _ = fullsize_inputs("nuscenes")
    probs = [cu(s[k]) for k in ("pr2d", "pr3d") for s in raw]
    labels = [cu(s[k]) for k in ("pl2d", "pl3d") for s in raw]
    assert len(labels) == 32
    got = sp.refine_pseudo_labels_segmented(probs, labels, num_classes=FULL_CLASSES)
    for p, l, o in zip(probs, labels, got):
        want = refine_pseudo_labels(p, l, num_classes=FULL_CLASSES)
        assert o.dtype == torch.int64 and torch.equal(o, want) and bool((o == -100).any())
    # unequal lengths, an empty segment, a one-point segment, labels outside [0, C) pass through, the default class count
    rng = np.random.Generator(np.random.PCG64(5))
    ns = [1000, 0, 1, 4097, 333, 2]
    probs = [cu(rng.random(n, dtype=np.float32) ** 0.3) for n in ns]
    labels = [cu(rng.integers(-1, 34, n)) for n in ns]
    got = sp.refine_pseudo_labels_segmented(probs, labels)
    for n, p, l, o in zip(ns, probs, labels, got):
        assert o.shape == (n,) and torch.equal(o, refine_pseudo_labels(p, l))
    cast = sp.refine_pseudo_labels_segmented(None, [l.to(torch.int16) for l in labels])
    assert all(torch.equal(a, l) for a, l in zip(cast, labels))


def fullsize_batch(name):
    from mopa_amd import scanprep as sp
    raw, mapping = fullsize_inputs(name)
    samples = []
    for s in raw:
        np.random.seed(s["draw_seed"])
        rot, u = sp.draw_augmentation_3d(**FULL_AUG)
        samples.append(device_sample(s, rot, u))
    batch = sp.prepare_batch_3d(samples, scale=20, full_scale=4096, label_mapping=cu(mapping), ema_input=True)
    return batch, cu(np.concatenate([s["pl3d"].astype(np.int64) for s in raw]))


@pytest.mark.parametrize("name", ["nuscenes", "kitti"])
def test_full_size_checksums_and_two_runs_give_identical_bits(name):
    want = json.load(open(os.path.join(GOLDEN, "g11_scanprep_fullsize.json")))[name]
    batch, teacher = fullsize_batch(name)
    check_structure(batch, 16)
    top, lists = batch_outputs(batch, teacher)
    assert [int(i.sum()) for i in lists["idxs"]] == want["kept"]
    for key, v in top.items():
        assert checksum(v) == want[key], key
    for key, ls in lists.items():
        assert checksum(np.concatenate([a.astype(np.uint8) if a.dtype == np.bool_ else a for a in ls])) == want[key], key
    again, _ = fullsize_batch(name)
    top2, lists2 = batch_outputs(again, teacher)
    assert all(np.array_equal(top[k], top2[k]) for k in top)
    assert all(np.array_equal(a, b) for k in lists for a, b in zip(lists[k], lists2[k]))


def test_batch_feeds_net3dseg_like_collate_scans_and_take_compacts_teacher_labels(g11):
    from mopa_amd import scanprep as sp
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_3d
    from mopa_amd.voxelize import collate_scans
    g, meta = g11
    k = [m["name"] for m in meta].index("partial")
    m = meta[k]
    batch, raw, samples = run_case(g, k, m, from_rotated=False)
    old = collate_scans([cu(s["points"]) for s in raw], m["scale"], m["full_scale"], [s.get("u") for s in raw])
    assert torch.equal(batch["x"][0], old[0]) and torch.equal(batch["x"][1], old[1])
    torch.manual_seed(0)
    cfg = default_cfg()
    cfg.MODEL_3D.SCN.num_planes = 4
    model = build_model_3d(cfg)[0].cuda().eval()
    with torch.no_grad():
        a = model({"x": batch["x"]})["seg_logit"]
        b = model({"x": old})["seg_logit"]
    assert a.shape[0] == batch["x"][0].shape[0] and torch.equal(a, b)
    for name in ("keep_in", "collate4", "partial"):
        k = [mm["name"] for mm in meta].index(name)
        batch, raw, _ = run_case(g, k, meta[k], from_rotated=False)
        teacher = cu(np.concatenate([s["teacher"] for s in raw]))
        assert np.array_equal(np_(sp.take(batch, teacher)), g[f"c{k}_taken"]), name


def sync_warnings(fn):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        fn()
    return [x for x in w if "synchroniz" in str(x.message).lower()]


@pytest.mark.parametrize("B", [2, 16])
def test_host_synchronisation_contract(B):
    from mopa_amd import scanprep as sp
    rng = np.random.Generator(np.random.PCG64(B))
    raw = []
    for b in range(B):
        n = 3000 + 17 * b
        raw.append({"points": (rng.standard_normal((n, 3)) * np.array([10.0, 10.0, 1.0])).astype(np.float32),
                    "seg_raw": rng.integers(0, 5, n).astype(np.uint8), "img": rng.integers(0, 40, (n, 2)).astype(np.int64),
                    "pl2d": rng.integers(0, 5, n).astype(np.int32), "pr2d": rng.random(n, dtype=np.float32),
                    "pl3d": rng.integers(0, 5, n).astype(np.int32), "pr3d": rng.random(n, dtype=np.float32),
                    "keep_in": rng.random(n) < 0.5})
    np.random.seed(B)
    draws = [sp.draw_augmentation_3d(0.1, 0.5, 0.0, 6.2831, True) for _ in range(B)]
    plain = [{k: v for k, v in device_sample(s, r, u).items() if k != "keep_in"} for s, (r, u) in zip(raw, draws)]
    crop = [device_sample(s, r, u) for s, (r, u) in zip(raw, draws)]
    forms = {"inside": lambda: sp.prepare_batch_3d(plain, 20, 4096, ema_input=True, assume_inside=True),
             "general": lambda: sp.prepare_batch_3d(plain, 20, 4096, ema_input=True),
             "keep_in": lambda: sp.prepare_batch_3d(crop, 20, 4096, ema_input=True)}
    for fn in forms.values():       # warm-up: library load, workspace and allocator growth
        fn()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        inside = forms["inside"]()
        torch.cuda.set_sync_debug_mode("warn")
        counts = {name: len(sync_warnings(forms[name])) for name in ("general", "keep_in")}
        none = len(sync_warnings(forms["inside"]))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert counts == {"general": 1, "keep_in": 1} and none == 0, (counts, none)
    general = forms["general"]()
    assert int(inside["n_outside"]) == 0 and torch.equal(inside["x"][0], general["x"][0])
    assert torch.equal(inside["ori_x"][0], general["ori_x"][0]) and torch.equal(inside["seg_label"], general["seg_label"])
    assert torch.equal(inside["pseudo_label_3d"], general["pseudo_label_3d"]) and torch.equal(inside["gather"], general["gather"])
    assert all(torch.equal(a, b) for a, b in zip(inside["aug_points_ls"], general["aug_points_ls"]))


def test_assume_inside_emits_and_counts_coordinates_outside_the_field():
    from mopa_amd import scanprep as sp
    pts = torch.zeros(100, 3, device="cuda")
    pts[:3, 0] = 300.0                                     # 6000 voxels from the minimum
    batch = sp.prepare_batch_3d([{"points": pts}, {"points": pts[3:]}], 20, 4096, assume_inside=True)
    assert int(batch["n_outside"]) == 3 and batch["x"][0].shape == (197, 4) and int(batch["x"][0][:, 0].max()) == 6000
    kept = sp.prepare_batch_3d([{"points": pts}, {"points": pts[3:]}], 20, 4096)
    assert kept["x"][0].shape == (194, 4) and np_(kept["offsets"]).tolist() == [0, 97, 194]


def test_launch_count_does_not_depend_on_the_batch_size(monkeypatch):
    from mopa_amd import _lib
    from mopa_amd import scanprep as sp
    raw, mapping = fullsize_inputs("kitti", B=16)
    raw = [{k: (v[:5000] if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in raw]
    calls = []
    real = _lib.call
    monkeypatch.setattr(sp, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    counts = {}
    for form in ("general", "keep_in", "inside"):
        for B in (2, 16):
            samples = [device_sample(s, np.diag([1, -1, 1]).astype(np.float32), np.full(3, 0.5)) for s in raw[:B]]
            if form != "keep_in":
                samples = [{k: v for k, v in d.items() if k != "keep_in"} for d in samples]
            del calls[:]
            sp.prepare_batch_3d(samples, 20, 4096, label_mapping=cu(mapping), ema_input=True, assume_inside=form == "inside")
            counts[form, B] = list(calls)
        assert counts[form, 2] == counts[form, 16], form
        assert 0 < len(counts[form, 2]) <= 7, counts[form, 2]


def test_c_abi_refuses_malformed_calls():
    import ctypes
    from mopa_amd import _lib
    lib = _lib.load()
    pts = torch.zeros(8, 3, device="cuda")
    lab = torch.zeros(8, dtype=torch.int64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    src, n1, neg = (ctypes.c_void_p * 1)(pts.data_ptr()), (ctypes.c_int32 * 1)(8), (ctypes.c_int32 * 1)(-1)
    labs, outs = (ctypes.c_void_p * 1)(lab.data_ptr()), (ctypes.c_void_p * 1)(lab.data_ptr())
    P = ctypes.addressof
    st = _lib.stream()
    assert lib.mopa_scanprep_count(None, None, P(n1), None, None, 1, 1, 20.0, 4096, 0, None, None, ws.data_ptr(), ws.numel(), st) == -1
    assert lib.mopa_scanprep_count(P(src), None, P(neg), None, None, 1, 1, 20.0, 4096, 0, None, None, ws.data_ptr(), ws.numel(), st) == -1
    assert lib.mopa_scanprep_count(P(src), None, P(n1), None, None, 1, 1, 20.0, 4096, 0, None, None, None, ws.numel(), st) == -1
    assert lib.mopa_scanprep_count(P(src), None, P(n1), None, None, 1, 1, 20.0, 4096, 0, None, None, ws.data_ptr(), 16, st) == -2
    assert lib.mopa_scanprep_count(P(src), None, P(n1), None, None, 1, 1, 20.0, 4096, 0, None, None, ws.data_ptr(), ws.numel(), st) == 0
    assert lib.mopa_scanprep_compact(P(src), None, P(n1), None, None, 1, 1, 0, 20.0, 4096, 1, None, None, None, None, 0, None, None, None,
                                     ws.data_ptr(), ws.numel(), st) == -1
    assert lib.mopa_refine_pseudo_labels_segmented(None, P(labs), 3, P(n1), P(outs), 1, 33, -100, ws.data_ptr(), ws.numel(), st) == -1
    assert lib.mopa_refine_pseudo_labels_segmented(None, P(labs), 3, P(n1), P(outs), 1, 8, -100, ws.data_ptr(), 16, st) == -2
    assert lib.mopa_refine_pseudo_labels_segmented(None, None, 3, P(n1), P(outs), 1, 8, -100, ws.data_ptr(), ws.numel(), st) == -1
    assert lib.mopa_refine_pseudo_labels_segmented(None, P(labs), 3, P(neg), P(outs), 1, 8, -100, ws.data_ptr(), ws.numel(), st) == -1
    assert lib.mopa_refine_pseudo_labels_segmented(None, P(labs), 3, P(n1), P(outs), 1, 8, -100, ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
