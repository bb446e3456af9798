"""Fixture G15 (tests/golden_gen/g15_nuscprep.py: the reference's map_pointcloud_to_image run on the host) is what
csrc/nuscprep.hip states it is -- the elementwise restatement of tests/_nuscenes_reference.py (fused chains, exact fma) gives
every bit of it --, the binding's host-side proj_matrix is the reference's, and every argument check of mopa_amd/nuscprep.py names
its argument before anything is launched.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import _nuscenes_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


@pytest.fixture(scope="module")
def g15():
    g = np.load(os.path.join(GOLDEN, "g15_nuscprep.npz"))
    return g, json.loads(str(g["meta"]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != F32:
        return bool((a == b).all())
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_exact_fma_rounds_once():
    """fma(a, b, c) where a * b + c rounded twice gives another float64."""
    a, b, c = 1 + 2.0 ** -30, 1 + 2.0 ** -30, -(1 + 2.0 ** -29)
    assert ref.fma(a, b, c) == 2.0 ** -60 and a * b + c == 0.0
    assert ref.fma(3.0, 4.0, 5.0) == 17.0 and np.isnan(ref.fma(np.inf, 0.0, 1.0)) and ref.fma(np.inf, 1.0, 1.0) == np.inf
    assert ref.chain([1.0, 2.0, 3.0], [4.0, 5.0, 6.0]) == 32.0


def test_fixture_loads(g15):
    g, meta = g15
    assert meta["rows"] == 1024 and meta["lds_boxes"] == 64
    assert [c["name"] for c in meta["cases"]] == ["realistic", "sizes", "exact", "ground_idx", "ground_mask"]
    sizes = meta["cases"][1]
    assert [len(g[f"c1_s{b}_scan"]) for b in range(5)] == [2 * 1024 + 3, 0, 1, 300, 700]
    assert [len(g[f"c1_s{b}_boxes"]) for b in range(5)] == [0, 3, 1, 2, 65] and sizes["counts"][1:4] == [0, 1, 0]
    assert [len(g[f"c0_s{b}_scan"]) for b in range(3)] == [1023, 1024, 1025]
    q = g["c0_s0_calib"][4:8]
    assert abs(1 - q @ q) > 1e-14                           # the one quaternion that is normalised on the way
    assert all(abs(1 - g["c0_s1_calib"][4 * j:4 * j + 4] @ g["c0_s1_calib"][4 * j:4 * j + 4]) < 1e-14 for j in range(4))


@pytest.mark.parametrize("k", range(5))
def test_the_restatement_gives_the_fixture_bit_for_bit(g15, k):
    g, meta = g15
    case = meta["cases"][k]
    for b in range(case["B"]):
        p = f"c{k}_s{b}_"
        kw = {"g": g[p + "g"]} if case["ground"] == "g_indices" else {"g_mask": g[p + "gmask"]} if case["ground"] == "g_mask" else {}
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            out = ref.preprocess_scan(g[p + "scan"], ref.unpack_calib(g[p + "calib"]), g[p + "boxes"], g[p + "box_class"],
                                      tuple(case["image_size"]), **kw)
        assert set(out) == {"points", "points_img", "seg_labels", "valid_mask"} | ({"g_indices"} if kw else set())
        for key, v in out.items():
            assert same_bits(v, g[p + key]), (case["name"], b, key)
        assert len(out["points"]) == case["counts"][b]


def test_exact_case_edges(g15):
    g, meta = g15
    k = [c["name"] for c in meta["cases"]].index("exact")
    notes = meta["cases"][k]["edges"]
    keep = g[f"c{k}_s2_valid_mask"]
    assert len(notes) == len(keep)
    for note, kept in zip(notes, keep):
        assert kept == (("kept" in note) or ("inside" in note) or ("outside" in note) or ("off the corner" in note)), note
    labels = g[f"c{k}_s2_seg_labels"]
    want = [3 if "inside" in n else ref.NO_BOX for n, kept in zip(notes, keep) if kept]
    assert labels.tolist() == want


def test_proj_matrix_of_the_binding_is_the_references(g15):
    """Five 4-term float64 products carry a few 1e-16 relative: three orders of margin, independent of the host's BLAS."""
    from mopa_amd.nuscprep import proj_matrix, rotation_matrix
    g, meta = g15
    for k, case in enumerate(meta["cases"]):
        for b in range(case["B"]):
            want = g[f"c{k}_s{b}_proj_matrix"]
            got = proj_matrix(ref.unpack_calib(g[f"c{k}_s{b}_calib"]))
            assert got.shape == (4, 4) and got.dtype == np.float64
            assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max()), (case["name"], b)
    R = rotation_matrix([0.5, -0.5, 0.5, -0.5])
    assert np.array_equal(R, [[0, 0, 1], [-1, 0, 0], [0, -1, 0]])
    assert np.allclose(rotation_matrix([2, 0, 0, 0]), np.eye(3))          # normalised on the way


# ---------------------------------------------------------------------------- argument refusals (CPU tensors: nothing is launched)
def good(n=8, m=2):
    rng = np.random.Generator(np.random.PCG64(3))
    calib = ref.nusc_calib(rng)
    boxes, cls = ref.view_boxes(rng, calib, m)
    return {"scan": torch.zeros(n, 5), "calib": calib, "boxes": boxes, "box_class": cls}


def refuse(exc, match, samples, *a, **kw):
    from mopa_amd.nuscprep import prepare_scans_nuscenes
    with pytest.raises(exc, match=match):
        prepare_scans_nuscenes(samples, *a, **kw)


def test_a_well_formed_call_on_the_cpu_is_refused_for_the_device_only():
    refuse(RuntimeError, "scan must be on the GPU", [good()])
    refuse(RuntimeError, "scan must be on the GPU", [dict(good(), g_mask=torch.zeros(8, dtype=torch.bool))])
    refuse(RuntimeError, "scan must be on the GPU", [dict(good(), boxes=np.zeros((0, 10)), box_class=np.zeros(0, np.int64))])
    refuse(RuntimeError, "scan must be on the GPU", [dict(good(), boxes=[], box_class=[])])


def test_argument_refusals_name_the_argument():
    refuse(ValueError, "no samples", [])
    refuse(ValueError, "image_size", [good()], image_size=(1600,))
    refuse(ValueError, "image_size", [good()], image_size=(0, 900))
    refuse(ValueError, "image_size", [good()], image_size=(1 << 24, 900))
    refuse(TypeError, "every sample must be a dict", [None])
    refuse(TypeError, "scan of sample 0 must be a torch tensor", [dict(good(), scan=np.zeros((8, 5), F32))])
    refuse(TypeError, "scan must be float32", [dict(good(), scan=torch.zeros(8, 5, dtype=torch.float64))])
    refuse(ValueError, "scan of sample 1 must be", [good(), dict(good(), scan=torch.zeros(8, 2))])
    refuse(ValueError, "scan of sample 0 must be", [dict(good(), scan=torch.zeros(40))])
    refuse(TypeError, "calib of sample 0 must be a dict", [dict(good(), calib=None)])
    for key in ref.CALIB_KEYS:
        c = dict(good()["calib"])
        del c[key]
        refuse(ValueError, f"lacks `{key}`", [dict(good(), calib=c)])
    c = dict(good()["calib"], cam_intrinsic=np.eye(4))
    refuse(ValueError, r"calib\['cam_intrinsic'\] of sample 0 must have shape \(3, 3\)", [dict(good(), calib=c)])
    c = dict(good()["calib"], lidar2ego_rotation=[1, 0, 0])
    refuse(ValueError, r"calib\['lidar2ego_rotation'\] of sample 0 must have shape \(4,\)", [dict(good(), calib=c)])
    c = dict(good()["calib"], cam2ego_rotation=[0, 0, 0, 0])
    refuse(ValueError, "zero quaternion", [dict(good(), calib=c)])
    c = dict(good()["calib"], cam2ego_translation=[0, float("nan"), 0])
    refuse(ValueError, "is not finite", [dict(good(), calib=c)])
    c = dict(good()["calib"], cam2ego_translation="abc")
    refuse(TypeError, r"calib\['cam2ego_translation'\]", [dict(good(), calib=c)])
    c = dict(good()["calib"], cam2ego_translation=torch.zeros(3))
    refuse(TypeError, "host list or numpy array", [dict(good(), calib=c)])
    refuse(TypeError, "boxes of sample 0 must be a host", [dict(good(), boxes=None)])
    refuse(TypeError, "boxes of sample 0 must be a host", [dict(good(), boxes=torch.zeros(2, 10))])
    refuse(ValueError, r"boxes of sample 0 must be \(M, 10\)", [dict(good(), boxes=np.zeros((2, 9)))])
    b = good()["boxes"].copy()
    b[1, 6:] = 0
    refuse(ValueError, "boxes of sample 0 hold a zero quaternion", [dict(good(), boxes=b)])
    b[1, 0] = np.inf
    refuse(ValueError, "boxes of sample 0 are not finite", [dict(good(), boxes=b)])
    refuse(TypeError, "box_class of sample 0 must be a host", [dict(good(), box_class=None)])
    refuse(TypeError, "box_class of sample 0 must be integers", [dict(good(), box_class=np.zeros(2))])
    refuse(ValueError, r"box_class of sample 0 must be \(2,\)", [dict(good(), box_class=np.zeros(3, np.int64))])
    refuse(ValueError, "box_class of sample 0 must lie in -1", [dict(good(), box_class=np.array([0, -2]))])
    refuse(ValueError, "box_class of sample 0 must lie in -1", [dict(good(), box_class=np.array([0, 256]))])
    g = torch.zeros(3, dtype=torch.int32)
    refuse(ValueError, "either every sample of a call has `g_indices` or none", [dict(good(), g_indices=g), good()])
    refuse(ValueError, "either every sample of a call has `g_mask` or none", [good(), dict(good(), g_mask=torch.zeros(8, dtype=torch.bool))])
    refuse(ValueError, "two forms of one input", [dict(good(), g_indices=g, g_mask=torch.zeros(8, dtype=torch.bool))])
    refuse(ValueError, "with_ground needs", [good()], with_ground=True)
    refuse(TypeError, "g_indices must be int32", [dict(good(), g_indices=g.long())])
    refuse(TypeError, "g_indices of sample 0 must be a torch tensor", [dict(good(), g_indices=np.zeros(3, np.int32))])
    refuse(ValueError, r"g_indices of sample 0 must be \(G,\)", [dict(good(), g_indices=g.reshape(1, 3))])
    refuse(TypeError, "g_mask must be bool", [dict(good(), g_mask=torch.zeros(8, dtype=torch.uint8))])
    refuse(ValueError, r"g_mask of sample 0 must be \(8,\)", [dict(good(), g_mask=torch.zeros(7, dtype=torch.bool))])


def test_types_are_named_before_the_device():
    """A malformed call is named as such on any device: the second sample's fault, not the first one's CPU tensor."""
    refuse(ValueError, "scan of sample 1 must be", [good(), dict(good(), scan=torch.zeros(8, 2))])
    refuse(TypeError, "box_class of sample 1", [good(), dict(good(), box_class=None)])

