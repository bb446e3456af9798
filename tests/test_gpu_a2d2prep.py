"""mopa_amd/a2d2prep.py on the device (csrc/a2d2prep.hip) against the numpy restatement tests/_a2d2_reference.py.  Every comparison
is an equality: torch.equal on integers and bytes, the bits on floats.

The cameras have A2D2's magnitude and are SYNTHETIC (tests/_a2d2_reference.py::CASES); OpenCV is not installed, so nothing here
was held against cv2.undistort.  What each case exercises is asserted on the restatement in tests/test_a2d2prep_host.py:
  identity        64 x 48, zero distortion, K' = K: frac == 0 everywhere; the last row / column have taps outside with weight 0
  barrel          96 x 64: no tap outside anywhere, shifts up to 9 px
  zoom_out        96 x 64, K' focal x 0.6: 21 % of the pixels wholly outside, 3.6 % partly
  odd_pincushion  67 x 45, x 0.7: 55 % wholly, 2.7 % partly, sx from -27 to 90, rows at every byte alignment
  tiny            33 x 17, x 0.5: 76 % wholly outside; full groups and a 1-pixel tail in every row
  rational        67 x 45, eight coefficients: the denominator is not 1
  contract        64 x 4, zero distortion, a camera found by search on which a chain contracted into fmas gives another map entry
                  than the chain rounded once per operation (the restatement): a contracted kernel fails the map comparison
  full size       1920 x 1208, B = 2: index width and grid coverage; map and image only
"""
import numpy as np
import pytest
import torch

import _a2d2_reference as ref

pytestmark = pytest.mark.gpu

NAMES = list(ref.CASES)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def equal(t, want):
    """torch.equal; float tensors by their bits."""
    t, want = t.cpu(), want if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    if t.dtype != want.dtype or t.shape != want.shape:
        return False
    return torch.equal(t.view(torch.int32), want.view(torch.int32)) if t.dtype == torch.float32 else torch.equal(t, want)


@pytest.fixture(scope="module")
def cases():
    """Per case: the restatement's map, the device's map, three noise images and their remaps by the restatement (computed once)."""
    from mopa_amd import a2d2prep as ap
    out = {}
    for k, (name, (W, H, cam)) in enumerate(ref.CASES.items()):
        rng = np.random.default_rng(100 + k)
        xy, frac = ref.undistort_map(cam, (W, H))
        imgs = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(3)]
        out[name] = {"W": W, "H": H, "cam": cam, "xy": xy, "frac": frac, "imgs": imgs, "want": [ref.remap(i, xy, frac) for i in imgs],
                     "umap": ap.undistort_map(cam, (W, H))}
    return out


def test_library_constants():
    from mopa_amd import _lib
    assert _lib.query("mopa_a2d2prep_max_frames") == 32 and _lib.query("mopa_a2d2prep_max_planes") == 64


@pytest.mark.parametrize("name", NAMES)
def test_map_equals_the_restatement(cases, name):
    c = cases[name]
    m = c["umap"]
    assert not m.identity and m.size == (c["W"], c["H"]) and m.xy.is_cuda and m.frac.is_cuda
    assert m.xy.dtype == torch.int16 and m.frac.dtype == torch.uint16
    assert equal(m.xy, c["xy"]) and equal(m.frac, c["frac"])


@pytest.mark.parametrize("name", NAMES)
def test_remap_equals_the_restatement_and_does_not_depend_on_the_batch(cases, name):
    from mopa_amd import a2d2prep as ap
    c = cases[name]
    dev = [cu(i) for i in c["imgs"]]
    names = []
    orig = ap.call
    ap.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
    try:
        together = ap.undistort_images(torch.stack(dev), c["umap"])
    finally:
        ap.call = orig
    assert names == ["mopa_a2d2prep_remap"]
    assert together.shape == (3, c["H"], c["W"], 3) and together.dtype == torch.uint8
    for b in range(3):
        assert equal(together[b], c["want"][b]), (name, b)
        alone = ap.undistort_images([dev[b]], c["umap"])
        assert alone.shape == (1, c["H"], c["W"], 3) and torch.equal(alone[0], together[b]), (name, b)
    # `out` is filled in place; one that overlaps an image is refused
    out = torch.full_like(together, 77)
    assert ap.undistort_images(dev, c["umap"], out=out) is out and torch.equal(out, together), name
    stacked = torch.stack(dev)
    with pytest.raises(ValueError, match="out overlaps image 0"):
        ap.undistort_images(stacked, c["umap"], out=stacked)
    with pytest.raises(ValueError, match="out overlaps image 2"):
        ap.undistort_images([dev[0], dev[1], out[1]], c["umap"], out=out)
    if name == "identity":
        assert torch.equal(together, torch.stack(dev))


def test_full_size_map_and_two_images():
    from mopa_amd import a2d2prep as ap
    W, H, cam = ref.FULL
    xy, frac = ref.undistort_map(cam, (W, H))
    m = ap.undistort_map(cam, (W, H))
    assert equal(m.xy, xy) and equal(m.frac, frac)
    rng = np.random.default_rng(7)
    imgs = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
    got = ap.undistort_images(cu(np.stack(imgs)), m)
    for b in range(2):
        assert equal(got[b], ref.remap(imgs[b], xy, frac)), b


def test_a_lens_that_is_not_undistorted_passes_through():
    from mopa_amd import a2d2prep as ap
    W, H, cam = ref.CASES["barrel"]
    m = ap.undistort_map(dict(cam, Lens="Pinhole"), (W, H))
    imgs = cu(np.random.default_rng(8).integers(0, 256, (2, H, W, 3)).astype(np.uint8))
    names = []
    orig = ap.call
    ap.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
    try:
        assert torch.equal(ap.undistort_images(imgs, m), imgs)
        s = frame_samples(np.random.default_rng(9), W, H, [5], "uint8")
        res = ap.prepare_frames_a2d2(dev_samples(s), m, cu(ref.TABLE), with_label_image=True)
    finally:
        ap.call = orig
    assert names == ["mopa_a2d2prep_points"]
    assert equal(res["img"][0], s[0]["image"]) and equal(res["label_img"][0], s[0]["label_image"])
    want = ref.prepare_frame(s[0]["label_image"], s[0]["points"], s[0]["row"], s[0]["col"], s[0]["reflectance"], ref.TABLE)
    assert equal(res["seg_labels"][0], want[2])


# ------------------------------------------------------------------------------------------------ the frames
def frame_samples(rng, W, H, ns, refl, n_bad=0, f32_points=False):
    out = []
    for n in ns:
        pts, row, col, r = ref.lidar_points(rng, n, W, H, n_bad=n_bad if n >= 4 else 0)
        if n >= 4:
            row[0], col[0] = -0.5, 0.75                    # truncation towards zero: pixel (0, 0), inside
        s = {"image": rng.integers(0, 256, (H, W, 3)).astype(np.uint8), "label_image": ref.block_labels(W, H),
             "points": pts.astype(np.float32) if f32_points else pts, "row": row, "col": col,
             "reflectance": None if refl is None else r if refl == "uint8" else (r / 3.0).astype(refl)}
        out.append(s)
    return out


def dev_samples(samples):
    return [{k: cu(v) for k, v in s.items() if v is not None} for s in samples]


def check_frames(res, samples, xy, frac, with_label_image, n_bad):
    K = len(ref.TABLE)
    B = len(samples)
    assert set(res) == {"img", "points", "feats", "seg_labels", "points_img", "bad_index"} | ({"label_img"} if with_label_image else set())
    assert res["bad_index"].is_cuda and res["bad_index"].dtype == torch.int32 and res["bad_index"].shape == (B,)
    real = ignore = total = 0
    for b, s in enumerate(samples):
        und = ref.remap(s["label_image"], xy, frac)
        p, f, seg, pimg, bad = ref.prepare_frame(und, s["points"], s["row"], s["col"], s["reflectance"], ref.TABLE)
        assert equal(res["img"][b], ref.remap(s["image"], xy, frac)), b
        for key, want in (("points", p), ("feats", f), ("seg_labels", seg), ("points_img", pimg)):
            t = res[key][b]
            assert t.is_cuda and t.shape == want.shape and equal(t, want), (key, b, t.shape, want.shape)
        assert int(res["bad_index"][b]) == bad == (n_bad if len(seg) >= 4 else 0)
        if with_label_image:
            assert equal(res["label_img"][b], und), b
            # the point kernel's pixel computed on the spot against a gather from the full plane
            r, c = s["row"].astype(np.int32), s["col"].astype(np.int32)
            ok = cu((r >= 0) & (r < und.shape[0]) & (c >= 0) & (c < und.shape[1]))
            px = res["label_img"][b][cu(r).long().clamp(0, und.shape[0] - 1), cu(c).long().clamp(0, und.shape[1] - 1)]
            hit = (px[:, None, :] == cu(ref.TABLE)[None]).all(2)
            last = torch.where(hit.any(1), K - 1 - hit.flip(1).int().argmax(1), K)
            assert torch.equal(res["seg_labels"][b], torch.where(ok, last, K).to(torch.uint8)), b
        inside = seg[:len(seg) - bad] if bad else seg
        real, ignore, total = real + int((inside != K).sum()), ignore + int((inside == K).sum()), total + len(inside)
    return real, ignore, total


@pytest.mark.parametrize("name", ["barrel", "odd_pincushion"])
@pytest.mark.parametrize("refl", ["uint8", "float64", None])
def test_frames_equal_the_restatement(cases, name, refl):
    from mopa_amd import a2d2prep as ap
    c = cases[name]
    rng = np.random.default_rng(11)
    samples = frame_samples(rng, c["W"], c["H"], [0, 1, 257, 3000], refl, n_bad=2)
    table = cu(ref.TABLE)
    names = []
    orig = ap.call
    ap.call = lambda nm, *a: (names.append(nm), orig(nm, *a))[1]
    try:
        res = ap.prepare_frames_a2d2(dev_samples(samples), c["umap"], table, with_label_image=True)
        assert names == ["mopa_a2d2prep_remap", "mopa_a2d2prep_points"]     # two launches for the four frames ...
        del names[:]
        one = ap.prepare_frames_a2d2(dev_samples(samples[3:]), c["umap"], table)
        assert names == ["mopa_a2d2prep_remap", "mopa_a2d2prep_points"]     # ... and for one
    finally:
        ap.call = orig
    real, ignore, total = check_frames(res, samples, c["xy"], c["frac"], True, 2)
    assert real >= 0.8 * total and ignore >= 0.01 * total, (real, ignore, total)
    if refl is None:
        assert all(f.dim() == 2 and f.shape[1] == 1 and bool((f == 1).all()) for f in res["feats"])
    # a frame gives the same whatever its neighbours in the call are; and without the label plane
    assert "label_img" not in one
    for key in ("points", "feats", "seg_labels", "points_img"):
        assert equal(one[key][0], res[key][3].cpu()), key
    assert torch.equal(one["img"][0], res["img"][3]) and int(one["bad_index"][0]) == 2


def test_float32_points_float32_reflectance_and_empty_call(cases):
    from mopa_amd import a2d2prep as ap
    c = cases["barrel"]
    samples = frame_samples(np.random.default_rng(12), c["W"], c["H"], [300, 2], np.float32, f32_points=True)
    res = ap.prepare_frames_a2d2(dev_samples(samples), c["umap"], cu(ref.TABLE))
    check_frames(res, samples, c["xy"], c["frac"], False, 0)
    empty = frame_samples(np.random.default_rng(13), c["W"], c["H"], [0, 0], "uint8")
    res = ap.prepare_frames_a2d2(dev_samples(empty), c["umap"], cu(ref.TABLE))
    check_frames(res, empty, c["xy"], c["frac"], False, 0)
    assert res["bad_index"].tolist() == [0, 0] and res["points"][0].shape == (0, 3) and res["feats"][1].shape == (0,)


def test_validate_labels_names_the_frame(cases, monkeypatch):
    from mopa_amd import a2d2prep as ap
    c = cases["barrel"]
    samples = frame_samples(np.random.default_rng(14), c["W"], c["H"], [10], "uint8") + \
        frame_samples(np.random.default_rng(15), c["W"], c["H"], [10], "uint8", n_bad=2)
    monkeypatch.setenv("MOPA_VALIDATE_LABELS", "1")
    with pytest.raises(IndexError, match="2 points of sample 1"):
        ap.prepare_frames_a2d2(dev_samples(samples), c["umap"], cu(ref.TABLE))
    ap.prepare_frames_a2d2(dev_samples(samples[:1]), c["umap"], cu(ref.TABLE))
    monkeypatch.delenv("MOPA_VALIDATE_LABELS")
    assert ap.prepare_frames_a2d2(dev_samples(samples), c["umap"], cu(ref.TABLE))["bad_index"].tolist() == [0, 2]


def test_chain_into_the_batch_preparation(cases):
    """img and points_img go into imageprep.prepare_batch (resize form), points and seg_labels into scanprep.prepare_batch_3d, as
    they come."""
    from mopa_amd import a2d2prep as ap, imageprep, scanprep
    c = cases["barrel"]
    W, H = c["W"], c["H"]
    samples = frame_samples(np.random.default_rng(16), W, H, [400, 300], "uint8")
    for s in samples:
        s["row"][0] = 0.5                                  # the dataset's points lie inside the image
    res = ap.prepare_frames_a2d2(dev_samples(samples), c["umap"], cu(ref.TABLE))
    ns = [400, 300]
    b2 = imageprep.prepare_batch([{"image": res["img"][b], "points_img": res["points_img"][b], "flip": b == 1} for b in range(2)], resize=(48, 32))
    assert b2["img"].shape == (2, 3, 32, 48) and b2["img"].dtype == torch.float32 and bool(torch.isfinite(b2["img"]).all())
    assert [tuple(t.shape) for t in b2["img_indices"]] == [(n, 2) for n in ns]
    for t in b2["img_indices"]:
        assert t.dtype == torch.int64 and int(t.min()) >= 0 and int(t[:, 0].max()) < 32 and int(t[:, 1].max()) < 48
    b3 = scanprep.prepare_batch_3d([{"points": res["points"][b], "seg_label": res["seg_labels"][b], "img_indices": b2["img_indices"][b]}
                                    for b in range(2)], scale=20)
    M = b3["x"][0].shape[0]
    assert 0 < M <= sum(ns) and b3["seg_label"].shape == (M,) and b3["seg_label"].dtype == torch.int64
    want = torch.cat(res["seg_labels"]).to(torch.int64)[b3["gather"]]
    assert torch.equal(b3["seg_label"], want) and int(b3["seg_label"].max()) <= len(ref.TABLE)
