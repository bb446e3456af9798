"""mopa_amd/nuscprep.py on the device (csrc/nuscprep.hip) against fixture G15: the reference's map_pointcloud_to_image run on the
host, behind it the stated labelling loop of preprocess.py:116-126 (tests/golden_gen/g15_nuscprep.py).  Every comparison is an
equality (of the bits for float tensors).  Reads only committed fixtures.

The small cases (R = rows per block):
  realistic    B = 3, N = R - 1, R, R + 1; calibration of nuScenes magnitude, one quaternion off unit by more than 1e-14; 12 boxes,
               two overlapping with different classes, one without a class over labelled points
  sizes        B = 5, N = 2 R + 3 (no boxes), 0, 1 (kept), 300 behind the camera (Nk = 0 between non-empty scans), 700 with one
               box more than an LDS chunk
  exact        exact arithmetic in any order: points on u = 0, u = W, v = 0, v = H (excluded), a step inside (kept), depth 0 with
               a zero / positive / negative numerator, depth < 0, a NaN coordinate; points on a face, an edge and a corner of an
               axis-aligned box (inside), one float32 step outside; in the first block and straddling row R
  ground_idx   an index list with the first and last raw index, a repeat and a negative index; an empty list
  ground_mask  the mask form, on (N, 4) rows
"""
import json
import os

import numpy as np
import pytest
import torch

import _nuscenes_reference as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LISTS = ("points", "points_img", "seg_labels", "valid_mask", "g_indices")


@pytest.fixture(scope="module")
def g15():
    g = np.load(os.path.join(GOLDEN, "g15_nuscprep.npz"))
    return g, json.loads(str(g["meta"]))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_samples(g, k, case):
    out = []
    for b in range(case["B"]):
        p = f"c{k}_s{b}_"
        s = {"scan": cu(g[p + "scan"]), "calib": ref.unpack_calib(g[p + "calib"]), "boxes": g[p + "boxes"], "box_class": g[p + "box_class"]}
        if case["ground"] == "g_indices":
            s["g_indices"] = cu(g[p + "g"])
        if case["ground"] == "g_mask":
            s["g_mask"] = cu(g[p + "gmask"])
        out.append(s)
    return out


def equal(t, want):
    """torch.equal; float tensors by their bits."""
    t, want = t.cpu(), want if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    if t.dtype != want.dtype or t.shape != want.shape:
        return False
    return torch.equal(t.view(torch.int32), want.view(torch.int32)) if t.dtype == torch.float32 else torch.equal(t, want)


def check_case(g, k, case, res):
    want_keys = {"points", "points_img", "seg_labels", "valid_mask", "proj_matrix", "counts"} | ({"g_indices"} if case["ground"] else set())
    assert set(res) == want_keys
    assert isinstance(res["counts"], np.ndarray) and res["counts"].dtype == np.int64 and res["counts"].tolist() == case["counts"]
    for key in LISTS:
        if key not in res:
            continue
        assert len(res[key]) == case["B"]
        for b, t in enumerate(res[key]):
            want = torch.from_numpy(g[f"c{k}_s{b}_{key}"])
            assert t.is_cuda and t.dtype == want.dtype and t.shape == want.shape, (case["name"], key, b, t.dtype, t.shape, want.dtype, want.shape)
            assert equal(t, want), (case["name"], key, b)
    for b, m in enumerate(res["proj_matrix"]):
        want = g[f"c{k}_s{b}_proj_matrix"]
        assert isinstance(m, np.ndarray) and m.dtype == np.float64 and m.shape == (4, 4)
        assert np.allclose(m, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_library_constants_are_what_the_fixture_was_sized_for(g15):
    from mopa_amd import _lib
    assert _lib.query("mopa_nuscprep_rows_per_block") == g15[1]["rows"]
    assert _lib.query("mopa_nuscprep_max_boxes") == g15[1]["lds_boxes"]
    assert _lib.query("mopa_nuscprep_max_scans") == 32
    assert _lib.query("mopa_nuscprep_workspace_bytes", 10) > 0 and _lib.query("mopa_nuscprep_table_bytes", 2, 3) == (2 * 64 + 3 * 25) * 8


@pytest.mark.parametrize("k", range(5))
def test_small_cases_equal_the_reference(g15, k):
    from mopa_amd.nuscprep import prepare_scans_nuscenes
    g, meta = g15
    case = meta["cases"][k]
    samples = device_samples(g, k, case)
    res = prepare_scans_nuscenes(samples, tuple(case["image_size"]))
    check_case(g, k, case, res)
    if case["ground"]:                                  # with_ground=False leaves the ground out and changes nothing else
        again = prepare_scans_nuscenes(samples, tuple(case["image_size"]), with_ground=False)
        assert "g_indices" not in again
        for key in LISTS[:4]:
            assert all(equal(a, b.cpu()) for a, b in zip(res[key], again[key])), key


@pytest.mark.parametrize("name", ["sizes", "exact"])
def test_one_call_of_b_and_b_calls_of_one_give_the_same_bits(g15, name):
    """What a sample gives does not depend on its neighbours in the call; and the launch count does not depend on B or M."""
    from mopa_amd import nuscprep
    g, meta = g15
    k = [c["name"] for c in meta["cases"]].index(name)
    case = meta["cases"][k]
    samples = device_samples(g, k, case)
    names = []
    orig = nuscprep.call
    nuscprep.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
    try:
        together = nuscprep.prepare_scans_nuscenes(samples, tuple(case["image_size"]))
        assert names == ["mopa_nuscprep_setup", "mopa_nuscprep_count", "mopa_nuscprep_scatter"]
        for b, s in enumerate(samples):
            del names[:]
            res = nuscprep.prepare_scans_nuscenes([s], tuple(case["image_size"]))
            assert names == ["mopa_nuscprep_setup", "mopa_nuscprep_count", "mopa_nuscprep_scatter"]
            assert res["counts"].tolist() == [case["counts"][b]]
            for key in LISTS[:4]:
                assert equal(res[key][0], together[key][b].cpu()), (key, b)
                assert equal(res[key][0], g[f"c{k}_s{b}_{key}"]), (key, b)
    finally:
        nuscprep.call = orig


def test_more_scans_than_one_launch_takes(g15):
    """34 scans (the library takes 32 per launch): the call splits them, still with one read-back, same rows."""
    from mopa_amd import nuscprep
    g, meta = g15
    k = [c["name"] for c in meta["cases"]].index("ground_idx")
    case = meta["cases"][k]
    two = device_samples(g, k, case)
    order = [j % 2 for j in range(34)]
    names, reads = [], []
    orig = nuscprep.call
    nuscprep.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
    blocking = {nm: getattr(torch.Tensor, nm) for nm in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__index__")}
    own = set(vars(torch.Tensor))
    for nm, fn in blocking.items():                     # every way a device tensor's content reaches the host
        setattr(torch.Tensor, nm, (lambda fn, nm: lambda self, *a, **k: (reads.append(nm) if self.is_cuda else None, fn(self, *a, **k))[1])(fn, nm))
    try:
        res = nuscprep.prepare_scans_nuscenes([two[j] for j in order], tuple(case["image_size"]))
    finally:
        nuscprep.call = orig
        for nm, fn in blocking.items():
            setattr(torch.Tensor, nm, fn) if nm in own else delattr(torch.Tensor, nm)
    assert names == ["mopa_nuscprep_setup", "mopa_kittiprep_ground", "mopa_nuscprep_count"] * 2 + ["mopa_nuscprep_scatter"] * 2
    assert reads == ["cpu"]                             # exactly one blocking read-back, for both chunks together
    assert res["counts"].tolist() == [case["counts"][j] for j in order]
    for key in LISTS:
        for i, j in enumerate(order):
            assert equal(res[key][i], g[f"c{k}_s{j}_{key}"]), (key, i)


def test_a_ground_index_outside_its_scan_is_refused(g15):
    from mopa_amd.nuscprep import prepare_scans_nuscenes
    g, meta = g15
    k = [c["name"] for c in meta["cases"]].index("ground_idx")
    case = meta["cases"][k]
    samples = device_samples(g, k, case)
    n = samples[0]["scan"].shape[0]
    for bad in (n, -n - 1):
        outside = dict(samples[0], g_indices=torch.tensor([0, bad], dtype=torch.int32).cuda())
        with pytest.raises(IndexError, match="g_indices"):
            prepare_scans_nuscenes([outside, samples[1]], tuple(case["image_size"]))
    inside = dict(samples[0], g_indices=torch.tensor([0, -n, n - 1], dtype=torch.int32).cuda())
    assert int(prepare_scans_nuscenes([inside], tuple(case["image_size"]))["counts"][0]) == case["counts"][0]


def test_fullsize_sweeps_match_the_checksums():
    from mopa_amd.nuscprep import prepare_scans_nuscenes
    with open(os.path.join(GOLDEN, "g15_nuscprep_fullsize.json")) as f:
        want = json.load(f)
    samples = [{"scan": cu(s["scan"]), "calib": s["calib"], "boxes": s["boxes"], "box_class": s["box_class"], "g_indices": cu(s["g"])}
               for s in ref.fullsize_inputs()]
    res = prepare_scans_nuscenes(samples, ref.NUSC_SIZE)
    assert res["counts"].tolist() == want["kept"]
    assert [int((t != ref.NO_BOX).sum()) for t in res["seg_labels"]] == want["labelled"]
    for key in LISTS:
        flat = torch.cat(res[key])
        flat = flat.to(torch.uint8) if flat.dtype == torch.bool else flat
        assert ref.checksum(flat.cpu().numpy()) == want[key], key


def test_drop_in_front_of_imageprep_and_scanprep(g15):
    """The outputs go through imageprep.prepare_batch and scanprep.prepare_batch_3d without conversion (uint8 labels, float32
    [row, col] points) and give the same img_indices, locs and seg_label as the reference's host-made arrays."""
    from mopa_amd import imageprep as ip, scanprep as sp
    from mopa_amd.nuscprep import prepare_scans_nuscenes
    g, meta = g15
    k = [c["name"] for c in meta["cases"]].index("realistic")
    case = meta["cases"][k]
    W, H = case["image_size"]
    res = prepare_scans_nuscenes(device_samples(g, k, case), (W, H))
    rng = np.random.Generator(np.random.PCG64(7))
    images = [cu(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)) for _ in range(case["B"])]
    flips = [False, True, False]
    mapping = cu(np.arange(256, dtype=np.int64) % 6)

    def chain(points_img, points, seg):
        two = ip.prepare_batch([{"image": im, "points_img": p, "flip": f} for im, p, f in zip(images, points_img, flips)], resize=(400, 225))
        three = sp.prepare_batch_3d([{"points": p, "rot": None, "transl_u": None, "seg_label": s} for p, s in zip(points, seg)],
                                    20, 4096, label_mapping=mapping)
        return two["img_indices"], three["x"][0], three["seg_label"]

    got = chain(res["points_img"], res["points"], res["seg_labels"])
    host = chain(*[[cu(g[f"c{k}_s{b}_{key}"]) for b in range(case["B"])] for key in ("points_img", "points", "seg_labels")])
    assert all(torch.equal(a, b) for a, b in zip(got[0], host[0])) and sum(len(a) for a in got[0]) > 0
    assert torch.equal(got[1], host[1]) and torch.equal(got[2], host[2]) and len(got[1]) > 0
