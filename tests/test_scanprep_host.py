"""The written contract of mopa_amd/scanprep.py against fixture G11 (tests/golden_gen/g11_scanprep.py: the reference's
augment_and_scale_3d, refine_pseudo_labels and collate_scn_base run on the host), without a GPU: the draws replay the reference's
generator, a fresh numpy restatement of the pipeline reproduces every recorded array (so the fixture is self-consistent and can be
read without the reference), and malformed calls are refused before any library call."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g11():
    g = np.load(os.path.join(GOLDEN, "g11_scanprep.npz"))
    return g, json.loads(str(g["meta"]))


def sample_inputs(g, k, b):
    keys = ("points", "seg_raw", "img", "keep_in", "pl2d", "pr2d", "pl3d", "pr3d", "teacher", "rot", "u", "aug_full")
    return {key: g[f"c{k}_s{b}_{key}"] for key in keys if f"c{k}_s{b}_{key}" in g.files}


# ---------------------------------------------------------------------------- the pipeline restated in numpy
def refine_np(probs, labels, ignore=-100):
    """Per class present: labels whose probability is below min(lower median, 0.9) become ``ignore``."""
    out = labels.astype(np.int64).copy()
    for c in np.unique(labels):
        idx = np.flatnonzero(labels == c)
        p = probs[idx]
        thresh = min(np.sort(p)[(len(p) - 1) // 2], np.float32(0.9))
        out[idx[p < thresh]] = ignore
    return out


def voxelize_np(aug, scale, full_scale, u):
    """rint(aug * scale) in float32, minus the minimum, the translation through float64, int64 truncation, the field filter."""
    c = np.rint(aug * np.float32(scale)).astype(np.float32)
    c = c - c.min(0)
    if u is not None:
        t = np.maximum(np.float32(full_scale) - c.max(0) - np.float32(0.001), np.float32(0))
        c = (c.astype(np.float64) + t.astype(np.float64) * u).astype(np.float32)
    ci = c.astype(np.int64)
    return ci, (ci.min(1) >= 0) & (ci.max(1) < full_scale)


def pipeline_np(samples, mapping, scale, full_scale, ema):
    """-> (batch-level dict, per-sample lists) under the fixture's names, from the recorded rotated points."""
    top = {k: [] for k in ("locs", "seg_label", "ps2", "ps3", "taken")}
    if ema:
        top["ori_locs"] = []
    lists = {k: [] for k in ("img_out", "aug_out", "orig_seg", "idxs", "ori_ps3") + (("ori_keep",) if ema else ())}
    for b, s in enumerate(samples):
        n = len(s["points"])
        keep = s["keep_in"] if "keep_in" in s else np.ones(n, bool)
        seg = (mapping[s["seg_raw"]] if mapping is not None else s["seg_raw"].astype(np.int64))[keep]
        ps2, ps3 = refine_np(s["pr2d"], s["pl2d"]), refine_np(s["pr3d"], s["pl3d"])
        if keep.any():
            ci, idxs = voxelize_np(s["aug_full"], scale, full_scale, s.get("u"))
        else:
            ci, idxs = np.zeros((0, 3), np.int64), np.zeros(0, bool)
        top["locs"].append(np.concatenate([ci[idxs], np.full((int(idxs.sum()), 1), b, np.int64)], 1))
        top["seg_label"].append(seg[idxs])
        top["ps2"].append(ps2[keep][idxs])
        top["ps3"].append(ps3[keep][idxs])
        top["taken"].append(s["teacher"][keep][idxs])
        lists["img_out"].append(s["img"][keep][idxs])
        lists["aug_out"].append(s["aug_full"][idxs])
        lists["orig_seg"].append(seg)
        lists["idxs"].append(idxs)
        lists["ori_ps3"].append(ps3)
        if ema:
            oc, oi = voxelize_np(s["points"], scale, full_scale, None)
            top["ori_locs"].append(np.concatenate([oc[oi], np.full((int(oi.sum()), 1), b, np.int64)], 1))
            lists["ori_keep"].append(keep)
    return {k: np.concatenate(v) for k, v in top.items()}, lists


def test_draws_replay_the_reference_generator(g11):
    from mopa_amd import scanprep as sp
    g, meta = g11
    for k, m in enumerate(meta):
        for b, seed in enumerate(m["seeds"]):
            np.random.seed(seed)
            rot, u = sp.draw_augmentation_3d(**m["aug"])
            assert np.random.rand() == float(g[f"c{k}_s{b}_next"])           # the generator is left where the reference leaves it
            for name, got in (("rot", rot), ("u", u)):
                key = f"c{k}_s{b}_{name}"
                assert (got is None) == (key not in g.files), (m["name"], name)
                if got is not None:
                    assert got.dtype == g[key].dtype and np.array_equal(got, g[key]), (m["name"], name)
    assert sp.draw_augmentation_3d() == (None, None)


def test_numpy_restatement_reproduces_every_fixture_array(g11):
    g, meta = g11
    names = [m["name"] for m in meta]
    for want in ("plain", "noisy_rot", "flip_x", "flip_y", "rot_z", "all", "noisy_rot_transl", "flip_x_transl", "flip_y_transl",
                 "rot_z_transl", "all_transl", "partial", "both_sides", "keep_in", "pseudo", "collate4"):
        assert want in names
    for k, m in enumerate(meta):
        samples = [sample_inputs(g, k, b) for b in range(m["B"])]
        mapping = g[f"c{k}_mapping"] if m["mapped"] else None
        top, lists = pipeline_np(samples, mapping, m["scale"], m["full_scale"], m["ema_input"])
        for key, v in top.items():
            assert v.dtype == g[f"c{k}_{key}"].dtype and np.array_equal(v, g[f"c{k}_{key}"]), (m["name"], key)
        for key, ls in lists.items():
            for b, v in enumerate(ls):
                ref = g[f"c{k}_s{b}_{key}"]
                assert v.shape == ref.shape and np.array_equal(v, ref), (m["name"], key, b)
        assert [int(i.sum()) for i in lists["idxs"]] == m["kept"]
        # the flips are exact in any BLAS: the recorded rotated points are the points with a sign
        if m["name"].startswith(("flip", "collate4", "keep_in")):
            for s in samples:
                if "rot" in s:
                    keep = s["keep_in"] if "keep_in" in s else np.ones(len(s["points"]), bool)
                    assert np.array_equal(s["aug_full"], s["points"][keep] * np.diag(s["rot"]))
    part = meta[names.index("partial")]
    assert 0 < part["kept"][0] < len(g[f"c{names.index('partial')}_s0_points"])
    kin = names.index("keep_in")
    assert not g[f"c{kin}_s1_keep_in"].any() and meta[kin]["kept"][1] == 0      # a scan whose crop mask is all false


def test_pseudo_label_cases_cover_what_they_claim(g11):
    g, meta = g11
    k = [m["name"] for m in meta].index("pseudo")
    a, b = sample_inputs(g, k, 0), sample_inputs(g, k, 1)
    assert 2 not in a["pl2d"] and 2 in b["pl2d"]                                 # a class absent from one scan
    counts = np.bincount(a["pl3d"])
    assert counts[0] % 2 == 0 and counts[1] % 2 == 1                             # an even and an odd class count
    assert np.median(b["pr2d"]) > 0.9 and (a["pr3d"] > 0.9).any()                # thresholds capped at 0.9
    assert (g[f"c{k}_ps2"] == -100).any() and (g[f"c{k}_ps3"] == -100).any()


def test_argument_errors_are_raised_before_any_library_call(monkeypatch):
    from mopa_amd import _lib
    from mopa_amd import scanprep as sp

    def boom(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(sp, "call", boom)
    monkeypatch.setattr(sp, "query", boom)
    pts = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.prepare_batch_3d([{"points": pts}], 20)
    with pytest.raises(TypeError):
        sp.prepare_batch_3d([{"points": pts.double()}], 20)
    with pytest.raises(TypeError):
        sp.prepare_batch_3d([{"points": pts.numpy()}], 20)
    with pytest.raises(ValueError):
        sp.prepare_batch_3d([{"points": torch.zeros(5, 4)}], 20)
    with pytest.raises(ValueError):
        sp.prepare_batch_3d([], 20)
    with pytest.raises(TypeError):
        sp.prepare_batch_3d([{"points": pts, "seg_label": torch.zeros(5)}], 20)                      # float labels
    with pytest.raises(TypeError):
        sp.prepare_batch_3d([{"points": pts, "keep_in": torch.zeros(5, dtype=torch.uint8)}], 20)     # the mask must be bool
    with pytest.raises(TypeError):
        sp.prepare_batch_3d([{"points": pts, "img_indices": torch.zeros(5, 2, dtype=torch.int32)}], 20)
    with pytest.raises(ValueError):
        sp.prepare_batch_3d([{"points": pts, "seg_label": torch.zeros(4, dtype=torch.int64)}], 20)   # mismatched lengths
    with pytest.raises(ValueError):
        sp.prepare_batch_3d([{"points": pts, "img_indices": torch.zeros(5, 3, dtype=torch.int64)}], 20)
    with pytest.raises(ValueError):
        sp.prepare_batch_3d([{"points": pts, "seg_label": torch.zeros(5, dtype=torch.int64)}, {"points": pts}], 20)   # all or none
    with pytest.raises(ValueError):
        sp.prepare_batch_3d([{"points": pts, "pseudo_label_2d": torch.zeros(5, dtype=torch.int64)}], 20)            # no probabilities
    with pytest.raises(ValueError):
        sp.prepare_batch_3d([{"points": pts, "rot": np.eye(2, dtype=np.float32)}], 20)
    with pytest.raises(ValueError):
        sp.prepare_batch_3d([{"points": pts, "transl_u": np.zeros(2)}], 20)
    with pytest.raises(TypeError):
        sp.prepare_batch_3d([{"points": pts, "seg_label": torch.zeros(5, dtype=torch.int64)}], 20, label_mapping=torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sp.refine_pseudo_labels_segmented([torch.zeros(4)], [torch.zeros(4, dtype=torch.int64)])


def test_c_abi_refuses_malformed_calls_on_the_host():
    """Every check is made before a launch: null tables, negative sizes, more than 32 classes, short workspaces."""
    import ctypes
    from mopa_amd import _lib
    lib = _lib.load()
    assert _lib.query("mopa_scanprep_workspace_bytes", 0) > 0 and _lib.query("mopa_scanprep_rows_per_block") > 0
    assert _lib.query("mopa_refine_pseudo_labels_segmented_workspace_bytes", 32, 32) >= 32 * 32 * 256 * 4
    assert _lib.query("mopa_refine_pseudo_labels_segmented_workspace_bytes", 0, 32) == 0
    one = (ctypes.c_void_p * 1)(4096)
    n1, neg = (ctypes.c_int32 * 1)(8), (ctypes.c_int32 * 1)(-1)
    P = ctypes.addressof
    assert lib.mopa_scanprep_rotate(None, P(one), P(n1), P(one), 1, None) == -1
    assert lib.mopa_scanprep_rotate(P(one), P(one), P(n1), P(one), 33, None) == -1
    assert lib.mopa_scanprep_count(None, None, P(n1), None, None, 1, 1, 20.0, 4096, 0, None, None, 4096, 1 << 20, None) == -1
    assert lib.mopa_scanprep_count(P(one), None, P(neg), None, None, 1, 1, 20.0, 4096, 0, None, None, 4096, 1 << 20, None) == -1
    assert lib.mopa_scanprep_count(P(one), None, P(n1), None, None, 1, 1, 20.0, 0, 0, None, None, 4096, 1 << 20, None) == -1
    assert lib.mopa_scanprep_count(P(one), None, P(n1), None, None, 1, 1, 20.0, 4096, 0, None, None, 4096, 16, None) == -2
    assert lib.mopa_scanprep_count(P(one), None, P(n1), None, None, 1, 1, 20.0, 4096, 1, None, None, 4096, 1 << 20, None) == -1
    assert lib.mopa_scanprep_compact(P(one), None, P(n1), None, None, 1, 1, 0, 20.0, 4096, 1, None, None, None, None, 0, None, None, None,
                                     4096, 1 << 20, None) == -1
    assert lib.mopa_scanprep_take(None, 0, 8, None, 1, None, 0, None, 0, -100, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.mopa_scanprep_take(None, 0, -1, P(n1), 1, None, 0, None, 0, -100, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.mopa_scanprep_take(None, 0, 8, P(n1), 1, None, 7, None, 0, -100, None, None, None, None, None, None, None, None, None, None) == -1
    args = (None, P(one), 3, P(n1), P(one), 1)
    assert lib.mopa_refine_pseudo_labels_segmented(*args, 33, -100, 4096, 1 << 24, None) == -1
    assert lib.mopa_refine_pseudo_labels_segmented(*args, 8, -100, 4096, 16, None) == -2
    assert lib.mopa_refine_pseudo_labels_segmented(None, None, 3, P(n1), P(one), 1, 8, -100, 4096, 1 << 24, None) == -1
    assert lib.mopa_refine_pseudo_labels_segmented(None, P(one), 3, P(neg), P(one), 1, 8, -100, 4096, 1 << 24, None) == -1
    assert lib.mopa_refine_pseudo_labels_segmented(None, P(one), 3, P(n1), P(one), 65, 8, -100, 4096, 1 << 24, None) == -1
