"""mopa_amd/kittiprep.py on the device against fixture G13 (the reference's SemanticKITTI preprocess and select_points_in_frustum
run on the host by tests/golden_gen/g13_kittiprep.py).  Every comparison is an equality (``torch.equal``; of the bits for float tensors, see ``equal``).  Reads only committed fixtures."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
LISTS = ("points", "feats", "seg_labels", "points_img", "ori_keep_idx", "g_indices", "full_scan", "all_seg_labels")


# ---------------------------------------------------------------------------- defined identically in tests/golden_gen/g13_kittiprep.py
def checksum(a) -> int:
    """Position-weighted sum of the array's bytes modulo 2^64."""
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).astype(np.uint64)
    return int((b * np.arange(1, b.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


# KITTI odometry sequence 00, calib.txt: P2 and Tr (public calibration)
P2 = np.array([[718.856, 0, 607.1928, 45.38225], [0, 718.856, 185.2157, -0.1130887], [0, 0, 1, 0.003779761]])
TR = np.array([[4.276802385584e-04, -9.999672484946e-01, -8.084491683471e-03, -1.198459927713e-02],
               [-7.210626507497e-03, 8.081198471645e-03, -9.999413164504e-01, -5.403984729748e-02],
               [9.999738645903e-01, 4.859485810390e-04, -7.206933692422e-03, -2.921968648686e-01], [0, 0, 0, 1]])
KITTI_SIZE = (1226, 370)
FULL = dict(B=4, n=120000, seed=131)


def kitti_proj():
    """proj_matrix as the dataset's pickle holds it (float64; preprocess casts it to float32)."""
    return P2 @ TR


def lidar_cloud(rng, n):
    """A 140 m x 140 m cloud around the sensor, z from below the -3 m cut to 2 m: about half in front, about a fifth in the image."""
    return np.stack([rng.uniform(-70, 70, n), rng.uniform(-70, 70, n), rng.uniform(-3.4, 2, n), rng.random(n)], 1).astype(F32)


def raw_labels(rng, n):
    """The .label file viewed as int32: a semantic id in the low 16 bits (some with bit 15 set), an instance id above them (some
    with bit 31 set)."""
    sem = rng.integers(0, 260, n).astype(np.uint32)
    sem[rng.random(n) < 0.1] |= 0x8000
    inst = rng.integers(0, 1 << 16, n).astype(np.uint32)
    return ((inst << 16) | sem).view(np.int32)


def fullsize_inputs():
    rng = np.random.Generator(np.random.PCG64(FULL["seed"]))
    out = []
    for b in range(FULL["B"]):
        n = FULL["n"]
        out.append({"scan": lidar_cloud(rng, n), "label": raw_labels(rng, n), "proj": kitti_proj(),
                    "g": np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)})
    return out
# ---------------------------------------------------------------------------- end of the shared part


@pytest.fixture(scope="module")
def g13():
    g = np.load(os.path.join(GOLDEN, "g13_kittiprep.npz"))
    return g, json.loads(str(g["meta"]))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_samples(g, k, case):
    out = []
    for b in range(case["B"]):
        p = f"c{k}_s{b}_"
        s = {"scan": cu(g[p + "scan"]), "label": cu(g[p + "label"])}
        if case["pseudo"]:
            s.update(ori_keep_idx=cu(g[p + "mask"]), ori_img_points=cu(g[p + "img_in"]))
        else:
            s["proj_matrix"] = g[p + "proj"]
        if case["with_g"]:
            s["g_indices"] = cu(g[p + "g"])
        out.append(s)
    return out


def equal(t, want):
    """torch.equal; float tensors by their bits, which asks more (the sign of a zero) and lets the NaN coordinates that the exact
    case carries through full_scan equal themselves."""
    t, want = t.cpu(), want if isinstance(want, torch.Tensor) else torch.from_numpy(want)
    if t.dtype != want.dtype or t.shape != want.shape:
        return False
    return torch.equal(t.view(torch.int32), want.view(torch.int32)) if t.dtype == torch.float32 else torch.equal(t, want)


def check_case(g, k, case, res):
    """torch.equal on every returned tensor against the reference's arrays, and the counts."""
    want_keys = {"points", "feats", "seg_labels", "points_img", "ori_keep_idx", "counts", "full_scan", "all_seg_labels"} | ({"g_indices"} if case["with_g"] else set())
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


def test_rows_per_block_is_what_the_fixture_was_sized_for(g13):
    from mopa_amd import _lib
    assert _lib.query("mopa_kittiprep_rows_per_block") == g13[1]["rows"]
    assert _lib.query("mopa_kittiprep_max_scans") == 32


@pytest.mark.parametrize("k", range(5))
def test_small_cases_equal_the_reference(g13, k):
    from mopa_amd.kittiprep import prepare_scans_kitti
    g, meta = g13
    case = meta["cases"][k]
    samples = device_samples(g, k, case)
    res = prepare_scans_kitti(samples, tuple(case["image_size"]), with_full=True)
    check_case(g, k, case, res)
    # a second run gives the same tensors; without with_full the two arrays are absent and the rest is unchanged
    again = prepare_scans_kitti(samples, tuple(case["image_size"]))
    assert "full_scan" not in again and "all_seg_labels" not in again
    for key in LISTS:
        if key in again:
            assert all(equal(a, b.cpu()) for a, b in zip(res[key], again[key])), key
    assert np.array_equal(res["counts"], again["counts"])
    if case["pseudo"]:                                  # the loaded image points are handed through, not projected
        assert all(a.data_ptr() == s["ori_img_points"].data_ptr() for a, s in zip(res["points_img"], samples))


def test_int64_labels_and_single_samples_give_the_same_rows(g13):
    """The same scans one per call and with int64 labels: what a sample gives does not depend on its neighbours in the call."""
    from mopa_amd.kittiprep import prepare_scans_kitti
    g, meta = g13
    k = [c["name"] for c in meta["cases"]].index("sizes")
    case = meta["cases"][k]
    for b, s in enumerate(device_samples(g, k, case)):
        s["label"] = s["label"].long()                  # sign-extended: the low 16 bits are the same
        res = prepare_scans_kitti([s], tuple(case["image_size"]), with_full=True)
        assert res["counts"].tolist() == [case["counts"][b]]
        for key in LISTS:
            assert equal(res[key][0], g[f"c{k}_s{b}_{key}"]), (key, b)


def test_an_empty_last_scan_changes_nothing_before_it(g13):
    """A call whose LAST scan is empty: the block table ends with two equal entries (the empty scan owns no block).  One block
    and one row of a second block, 300 rows, no rows -- each scan gives what it gives alone."""
    from mopa_amd import _lib
    from mopa_amd.kittiprep import prepare_scans_kitti
    g, meta = g13
    k = [c["name"] for c in meta["cases"]].index("sizes")
    case = meta["cases"][k]
    five = device_samples(g, k, case)
    rows = _lib.query("mopa_kittiprep_rows_per_block")
    assert [s["scan"].shape[0] for s in five][:4] == [2 * rows + 3, 0, 1, 300]
    cut = dict(five[0], scan=five[0]["scan"][:rows + 1], label=five[0]["label"][:rows + 1])
    samples = [{key: s[key] for key in ("scan", "label", "proj_matrix")} for s in (cut, five[3], five[1])]
    together = prepare_scans_kitti(samples, tuple(case["image_size"]), with_full=True)
    assert together["counts"][2].tolist() == [0, 0] and together["counts"][0, 0] > 0 and together["counts"][1, 0] > 0
    for b, s in enumerate(samples):
        alone = prepare_scans_kitti([s], tuple(case["image_size"]), with_full=True)
        assert alone["counts"].tolist() == [together["counts"][b].tolist()]
        for key in LISTS:
            if key != "g_indices":
                assert equal(together[key][b], alone[key][0].cpu()), (key, b)


def test_more_scans_than_one_launch_takes(g13):
    """34 scans (the library takes 32 per launch): the call splits them, still with one read-back, same rows."""
    from mopa_amd import kittiprep
    g, meta = g13
    k = [c["name"] for c in meta["cases"]].index("exact")
    case = meta["cases"][k]
    three = device_samples(g, k, case)
    order = [j % 3 for j in range(34)]
    names = []
    orig = kittiprep.call
    kittiprep.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
    try:
        res = kittiprep.prepare_scans_kitti([three[j] for j in order], tuple(case["image_size"]), with_full=True)
    finally:
        kittiprep.call = orig
    assert names == ["mopa_kittiprep_ground", "mopa_kittiprep_count"] * 2 + ["mopa_kittiprep_scatter"] * 2
    assert res["counts"].tolist() == [case["counts"][j] for j in order]
    for key in LISTS:
        for i, j in enumerate(order):
            assert equal(res[key][i], g[f"c{k}_s{j}_{key}"]), (key, i)


def test_what_only_the_counts_can_tell_is_refused(g13):
    from mopa_amd.kittiprep import prepare_scans_kitti
    g, meta = g13
    k = [c["name"] for c in meta["cases"]].index("pseudo")
    case = meta["cases"][k]
    samples = device_samples(g, k, case)
    short = dict(samples[1], ori_keep_idx=samples[1]["ori_keep_idx"][:-1])
    with pytest.raises(ValueError, match="ori_keep_idx of sample 1"):
        prepare_scans_kitti([samples[0], short], tuple(case["image_size"]))
    fewer = dict(samples[0], ori_img_points=samples[0]["ori_img_points"][:-1])
    with pytest.raises(ValueError, match="ori_img_points of sample 0"):
        prepare_scans_kitti([fewer, samples[1]], tuple(case["image_size"]))
    n = samples[0]["scan"].shape[0]
    outside = dict(samples[0], g_indices=torch.tensor([0, n], dtype=torch.int32).cuda())
    with pytest.raises(IndexError, match="g_indices"):
        prepare_scans_kitti([outside, samples[1]], tuple(case["image_size"]))


def test_fullsize_scans_match_the_checksums():
    from mopa_amd.kittiprep import prepare_scans_kitti
    with open(os.path.join(GOLDEN, "g13_kittiprep_fullsize.json")) as f:
        want = json.load(f)
    samples = [{"scan": cu(s["scan"]), "label": cu(s["label"]), "proj_matrix": s["proj"], "g_indices": cu(s["g"])} for s in fullsize_inputs()]
    res = prepare_scans_kitti(samples, KITTI_SIZE, with_full=True)
    assert res["counts"][:, 0].tolist() == want["nz"] and res["counts"][:, 1].tolist() == want["kept"]
    for key in LISTS:
        flat = torch.cat(res[key])
        flat = flat.to(torch.uint8) if flat.dtype == torch.bool else flat
        assert checksum(flat.cpu().numpy()) == want[key], key


def test_drop_in_front_of_imageprep_and_scanprep(g13):
    """A small case chained through imageprep.prepare_batch (crop form) and scanprep.prepare_batch_3d gives the same img_indices,
    locs and seg_label as feeding those two the reference's host-made preprocess outputs."""
    from mopa_amd import imageprep as ip, scanprep as sp
    from mopa_amd.kittiprep import prepare_scans_kitti
    g, meta = g13
    k = [c["name"] for c in meta["cases"]].index("realistic")
    case = meta["cases"][k]
    W, H = case["image_size"]
    res = prepare_scans_kitti(device_samples(g, k, case), (W, H))
    rng = np.random.Generator(np.random.PCG64(7))
    images = [cu(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)) for _ in range(case["B"])]
    crops = [(left, H - 302, left + 480, H) for left in (0, 373, W - 480)]
    flips = [False, True, False]
    mapping = cu(np.arange(1 << 15, dtype=np.int64) % 11)

    def chain(points_img, points, seg):
        two = ip.prepare_batch([{"image": im, "points_img": p, "crop": c, "flip": f} for im, p, c, f in zip(images, points_img, crops, flips)])
        assert all(int(kp.sum()) > 0 for kp in two["keep"])
        three = sp.prepare_batch_3d([{"points": p, "rot": None, "transl_u": None, "seg_label": s, "keep_in": kp}
                                     for p, s, kp in zip(points, seg, two["keep"])], 20, 4096, label_mapping=mapping)
        return two["img_indices"], three["x"][0], three["seg_label"]

    got = chain(res["points_img"], res["points"], res["seg_labels"])
    host = chain(*[[cu(g[f"c{k}_s{b}_{key}"]) for b in range(case["B"])] for key in ("points_img", "points", "seg_labels")])
    assert all(torch.equal(a, b) for a, b in zip(got[0], host[0])) and sum(len(a) for a in got[0]) > 0
    assert torch.equal(got[1], host[1]) and torch.equal(got[2], host[2]) and len(got[1]) > 0
