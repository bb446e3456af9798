"""mopa_amd/a2d2prep.py without a GPU: properties of the stated chain on its numpy restatement (tests/_a2d2_reference.py), the closed
form of the remap against cv2.remap's published 15-bit weight table, the coverage conditions that tests/test_gpu_a2d2prep.py
relies on (asserted here on the restatement, so that a changed case cannot quietly stop exercising a path), ``color_table``, and
every argument check, which names its argument before anything is launched.

OpenCV is not installed: nothing here ran cv2.  The cameras are synthetic (A2D2's magnitude, not the dataset's calibration)."""
import numpy as np
import pytest
import torch

import _a2d2_reference as ref
from mopa_amd import a2d2prep as ap


@pytest.fixture(scope="module")
def maps():
    return {name: ref.undistort_map(cam, (W, H)) for name, (W, H, cam) in ref.CASES.items()}


def shares(name, maps):
    W, H, _ = ref.CASES[name]
    xy, frac = maps[name]
    wholly, partly = ref.outside(xy, (W, H))
    return xy, frac, wholly.mean(), partly.mean()


# ------------------------------------------------------------------------------------------------ the chain
def test_zero_distortion_and_equal_matrices_give_the_image_back(maps):
    W, H, cam = ref.CASES["identity"]
    assert cam["CamMatrix"] == cam["CamMatrixOriginal"] and not np.any(cam["Distortion"])
    xy, frac = maps["identity"]
    assert xy.dtype == np.int16 and xy.shape == (H, W, 2) and frac.dtype == np.uint16 and frac.shape == (H, W)
    assert (frac == 0).all()
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    assert (xy[..., 0] == j).all() and (xy[..., 1] == i).all()
    img = np.random.default_rng(0).integers(0, 256, (H, W, 3)).astype(np.uint8)
    assert np.array_equal(ref.remap(img, xy, frac), img)
    # the last row and column have taps outside the source, all with weight 0: (W + H - 1) / (W H) = 3.6 %
    w0 = ref.partly_with_weight_zero(xy, frac, (W, H))
    assert w0.sum() == W + H - 1 and 0.035 < w0.mean() < 0.037


def test_closed_form_equals_the_15_bit_table_form():
    """All 1024 fractions x random taps, extremes included.  Both forms return p00 at frac = 0, where the table is
    [32767, 0, 0, 1]: 32767 p00 + p11 + 16384 = 32768 p00 + (16384 + p11 - p00) and 0 < 16384 + p11 - p00 < 32768."""
    tab = ref.table_weights()
    assert tab[0].tolist() == [32767, 0, 0, 1]
    assert (tab.sum(1) == 32768).all()
    w = np.stack(ref.weights(np.arange(1024, dtype=np.uint16)), 1)
    assert (tab[1:] == 32 * w[1:]).all() and w[0].tolist() == [1024, 0, 0, 0]
    rng = np.random.default_rng(1)
    taps = np.concatenate([rng.integers(0, 256, (24, 4)), [[0, 0, 0, 0], [255, 255, 255, 255], [0, 255, 255, 255], [255, 0, 0, 0],
                                                           [255, 0, 0, 255], [0, 0, 0, 255], [0, 255, 0, 255], [255, 0, 255, 0]]])
    for f in range(1024):
        closed = (taps @ w[f] + 512) >> 10
        table = [ref.remap_table_form(p, tab[f]) for p in taps]
        assert closed.tolist() == table, f
        if f == 0:
            assert closed.tolist() == taps[:, 0].tolist()


def test_fix32_rounds_half_to_even_and_saturates():
    u = np.array([0.5 / 32, 1.5 / 32, 2.5 / 32, -0.5 / 32, -1.5 / 32, 1e300, -1e300, np.inf, -np.inf, np.nan, 2.0 ** 26, -2.0 ** 26 - 1])
    assert ref.fix32(u).tolist() == [0, 2, 2, 0, -2, ref.I32_MAX, ref.I32_MIN, ref.I32_MIN, ref.I32_MIN, ref.I32_MIN, ref.I32_MAX, ref.I32_MIN]
    # a camera that sends every pixel far outside: the stored coordinates saturate to int16, and such a pixel is border
    W, H, cam = ref.CASES["barrel"]
    far = dict(cam, CamMatrixOriginal=[[80.0, 0.0, 1e8], [0.0, 80.0, -1e8], [0.0, 0.0, 1.0]])
    xy, frac = ref.undistort_map(far, (W, H))
    assert (xy[..., 0] == 32767).all() and (xy[..., 1] == -32768).all()
    assert not ref.remap(np.full((H, W, 3), 255, np.uint8), xy, frac).any()


def test_one_map_unit_moves_a_byte_by_at_most_8_levels():
    """The bound of DESIGN.md section 4: the fraction off by one unit (1/32 px) within the same 2 x 2 taps changes every weight
    by at most 32 of 1024, and at most 32 of 1024 of the weight moves from one tap pair to the other: ceil(255 / 32) = 8."""
    rng = np.random.default_rng(2)
    taps = np.concatenate([rng.integers(0, 256, (64, 4)), [[0, 255, 0, 255], [255, 0, 255, 0], [0, 0, 255, 255], [255, 255, 0, 0]]])
    w = np.stack(ref.weights(np.arange(1024, dtype=np.uint16)), 1)
    val = (taps @ w.T + 512) >> 10                        # (taps, 1024)
    val = val.reshape(len(taps), 32, 32)
    assert np.abs(np.diff(val, axis=1)).max() <= 8 and np.abs(np.diff(val, axis=2)).max() <= 8
    assert np.abs(np.diff(val, axis=2)).max() == 8        # and it is attained
    # across the footprint's edge: (sx, fx5 = 31) against (sx + 1, fx5 = 0), and (sy, fy5 = 31) against (sy + 1, 0), for every
    # fraction of the other axis, on an image whose every map entry is moved by that one unit
    img = rng.integers(0, 256, (12, 12, 3)).astype(np.uint8)
    img[::2, 1::2], img[1::2, ::2] = 0, 255                # neighbours 255 apart as well
    sy, sx = np.meshgrid(np.arange(-1, 12), np.arange(-1, 12), indexing="ij")      # the border's zero taps included
    for other in range(32):
        for axis in (0, 1):
            xy = np.stack([sx, sy], -1).astype(np.int16)
            lo = np.full(sx.shape, (other * 32 + 31) if axis == 0 else (31 * 32 + other), np.uint16)
            hi = np.full(sx.shape, (other * 32) if axis == 0 else other, np.uint16)
            xy_hi = xy.copy()
            xy_hi[..., axis] += 1
            d = np.abs(ref.remap(img, xy, lo).astype(np.int64) - ref.remap(img, xy_hi, hi).astype(np.int64))
            assert d.max() <= 8, (other, axis)


def test_contract_case_tells_a_contracted_chain_from_the_stated_one(maps):
    """The case `contract`: on its camera a chain whose u = fx * xd + cx is one fma gives another map entry than the chain
    rounded once per operation, so the device's map (compared with the latter in tests/test_gpu_a2d2prep.py) shows a kernel that
    the compiler contracted."""
    W, H, cam = ref.CASES["contract"]
    xy, frac = maps["contract"]
    stated = xy[0, :, 0].astype(np.int64) * 32 + (frac[0] & 31)
    fused = ref.fused_columns(cam, W)
    cols = np.flatnonzero(stated != fused)
    assert len(cols) >= 1 and cols.tolist() == ref.CONTRACT_COLUMNS.tolist()
    assert np.abs(stated - fused).max() == 1               # one unit of 1/32 px: a rounding tie of rint(u * 32)
    assert ref.fma(3.0, 4.0, 5.0) == 17.0 and ref.fma(1 + 2.0 ** -30, 1 + 2.0 ** -30, -(1 + 2.0 ** -29)) == 2.0 ** -60
    assert (xy[1:, :, 0] == xy[0, :, 0]).all()           # every row has the columns


# ------------------------------------------------------------------------------------------------ coverage of the GPU cases
def test_barrel_has_no_tap_outside_and_shifts_up_to_9_px(maps):
    W, H, _ = ref.CASES["barrel"]
    xy, frac, wholly, partly = shares("barrel", maps)
    assert wholly == 0 and partly == 0
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    assert max(np.abs(xy[..., 0] - j).max(), np.abs(xy[..., 1] - i).max()) == 9
    assert len(np.unique(frac)) > 900                      # nearly every fraction occurs


def test_zoom_out_odd_and_tiny_cover_the_border(maps):
    _, _, wholly, partly = shares("zoom_out", maps)
    assert 0.20 < wholly < 0.22 and 0.03 < partly < 0.04
    W, H, _ = ref.CASES["odd_pincushion"]
    xy, _, wholly, partly = shares("odd_pincushion", maps)
    assert 0.53 < wholly < 0.57 and 0.02 < partly < 0.035
    assert xy[..., 0].min() == -27 and xy[..., 0].max() == 90
    assert W % 4 and (W * 3) % 4                           # rows start at every byte alignment, a group is cut at the row's end
    W, H, _ = ref.CASES["tiny"]
    _, _, wholly, partly = shares("tiny", maps)
    assert 0.74 < wholly < 0.78 and partly > 0.03


def test_rational_case_has_a_denominator(maps):
    _, _, cam = ref.CASES["rational"]
    assert len(cam["Distortion"][0]) == 8 and all(cam["Distortion"][0][5:])
    _, _, wholly, partly = shares("rational", maps)
    assert partly >= 0.01 and wholly < 0.9
    five = dict(cam, Distortion=[cam["Distortion"][0][:5]])
    assert not np.array_equal(ref.undistort_map(five, (67, 45))[0], maps["rational"][0])


@pytest.mark.parametrize("name", ["barrel", "odd_pincushion"])
def test_label_pattern_reaches_both_branches(maps, name):
    W, H, _ = ref.CASES[name]
    K = len(ref.TABLE)
    assert K == 7 and ref.TABLE[6].tolist() == ref.TABLE[1].tolist() and len({tuple(r) for r in ref.TABLE.tolist()}) == 6
    assert not (ref.TABLE == np.array(ref.FOREIGN)).all(1).any()
    lab = ref.block_labels(W, H)
    assert (lab == np.array(ref.FOREIGN)).all(2).sum() == 64
    und = ref.remap(lab, *maps[name])
    cls = ref.classes(und.reshape(-1, 3), ref.TABLE)
    assert 0.04 < (cls == K).mean() < 0.10                 # the blended block borders and the foreign patch
    assert (cls == 6).any() and not (cls == 1).any()       # the last equal row wins
    # one map unit off, in x or in y, up or down, across the footprint's edge (fx5 = 31 -> sx + 1, fx5 = 0; 0 -> sx - 1, 31) too, never
    # turns one real class into another: between two classes lies a blend, which is class K
    xy, frac = maps[name]
    for axis in (0, 1):
        for step in (1, -1):
            fx, fy = frac.astype(np.int64) & 31, frac.astype(np.int64) >> 5
            pos = xy[..., axis].astype(np.int64) * 32 + (fx, fy)[axis] + step
            xy2 = xy.copy()
            xy2[..., axis] = pos >> 5
            moved = ((pos & 31) + fy * 32 if axis == 0 else (pos & 31) * 32 + fx).astype(np.uint16)
            assert ((xy2[..., axis] != xy[..., axis]).any())                    # the crossing occurs
            cls2 = ref.classes(ref.remap(lab, xy2, moved).reshape(-1, 3), ref.TABLE)
            differ = cls != cls2
            assert ((cls[differ] == K) | (cls2[differ] == K)).all(), (axis, step)


def test_prepare_frame_restatement():
    rng = np.random.default_rng(3)
    W, H = 96, 64
    und = ref.block_labels(W, H)
    pts, row, col, refl = ref.lidar_points(rng, 50, W, H, n_bad=2)
    row[0], col[0] = -0.5, 0.75                            # truncation towards zero: pixel (0, 0), inside
    p, f, seg, pimg, bad = ref.prepare_frame(und, pts, row, col, refl, ref.TABLE)
    assert bad == 2 and seg[-2:].tolist() == [7, 7] and seg[0] == ref.classes(und[0, :1], ref.TABLE)[0]
    assert p.dtype == f.dtype == pimg.dtype == np.float32 and seg.dtype == np.uint8 and f.shape == (50,) and pimg.shape == (50, 2)
    assert ref.prepare_frame(und, pts, row, col, None, ref.TABLE)[1].shape == (50, 1)


# ------------------------------------------------------------------------------------------------ color_table
def test_color_table_follows_file_order():
    t = ap.color_table({"#ff0000": "Car 1", "#00ff10": "Bicycle 1", "#0a0b0c": "Sky", "#FF0000": "again"})
    assert t.dtype == torch.uint8 and t.tolist() == [[255, 0, 0], [0, 255, 16], [10, 11, 12], [255, 0, 0]]
    for bad in ({}, [], {"ff00": "x"}, {"#gg0000": "x"}, {7: "x"}):
        with pytest.raises((TypeError, ValueError), match="color_table"):
            ap.color_table(bad)
    with pytest.raises(ValueError, match="at most 256"):
        ap.color_table({f"#{k:06x}": str(k) for k in range(257)})


def test_camera_params():
    _, _, cam = ref.CASES["rational"]
    p = ap.camera_params(cam)
    K = np.array(cam["CamMatrixOriginal"])
    Kn = np.array(cam["CamMatrix"])
    assert p.dtype == np.float64 and p.tolist() == [K[0, 0], K[1, 1], K[0, 2], K[1, 2], Kn[0, 0], Kn[1, 1], Kn[0, 2], Kn[1, 2]] + list(ref.DIST_RATIONAL)
    four = ap.camera_params(dict(cam, Distortion=[0.1, 0.2, 0.3, 0.4]))
    assert four[8:].tolist() == [0.1, 0.2, 0.3, 0.4, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ argument checks
def test_undistort_map_names_what_is_wrong():
    _, _, cam = ref.CASES["barrel"]
    with pytest.raises(NotImplementedError, match="Fisheye"):
        ap.undistort_map(dict(cam, Lens="Fisheye"), (96, 64))
    for n in (0, 3, 6, 7, 9, 12, 14):
        with pytest.raises(ValueError, match="Distortion"):
            ap.undistort_map(dict(cam, Distortion=[0.0] * n), (96, 64))
    with pytest.raises(ValueError, match="size"):
        ap.undistort_map(cam, (96,))
    with pytest.raises(ValueError, match="size"):
        ap.undistort_map(cam, (0, 64))
    with pytest.raises(ValueError, match="size"):
        ap.undistort_map(cam, (96, 40000))
    with pytest.raises(TypeError, match="camera"):
        ap.undistort_map([1, 2], (96, 64))
    with pytest.raises(ValueError, match="CamMatrixOriginal"):
        ap.undistort_map({k: v for k, v in cam.items() if k != "CamMatrixOriginal"}, (96, 64))
    with pytest.raises(ValueError, match="CamMatrix"):
        ap.undistort_map(dict(cam, CamMatrix=[[1.0, 0.0], [0.0, 1.0]]), (96, 64))
    with pytest.raises(ValueError, match="skew"):
        ap.undistort_map(dict(cam, CamMatrix=[[80.0, 0.1, 48.0], [0.0, 80.0, 32.0], [0.0, 0.0, 1.0]]), (96, 64))
    with pytest.raises(ValueError, match="focal"):
        ap.undistort_map(dict(cam, CamMatrix=[[0.0, 0.0, 48.0], [0.0, 80.0, 32.0], [0.0, 0.0, 1.0]]), (96, 64))
    with pytest.raises(ValueError, match="finite"):
        ap.undistort_map(dict(cam, Distortion=[0.0, np.nan, 0.0, 0.0]), (96, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ap.undistort_map(cam, (96, 64), device="cpu")


def test_other_lenses_pass_through_without_a_launch():
    _, _, cam = ref.CASES["barrel"]
    for lens in ("Pinhole", None, ""):
        m = ap.undistort_map(dict(cam, Lens=lens), (96, 64))
        assert m.identity and m.xy is None and m.frac is None and m.size == (96, 64)


def frame(n=5, W=96, H=64, **over):
    s = {"image": torch.zeros((H, W, 3), dtype=torch.uint8), "label_image": torch.zeros((H, W, 3), dtype=torch.uint8),
         "points": torch.zeros((n, 3), dtype=torch.float64), "row": torch.zeros(n, dtype=torch.float64),
         "col": torch.zeros(n, dtype=torch.float64)}
    s.update(over)
    return s


def test_calls_name_what_is_wrong_before_anything_is_launched():
    ident = ap.UndistortMap((96, 64), True)
    table = torch.zeros((7, 3), dtype=torch.uint8)
    f = ap.prepare_frames_a2d2
    with pytest.raises(ValueError, match="no samples"):
        f([], ident, table)
    with pytest.raises(TypeError, match="dict"):
        f([3], ident, table)
    with pytest.raises(TypeError, match="UndistortMap"):
        f([frame()], None, table)
    with pytest.raises(TypeError, match="image of sample 0"):
        f([frame(image=None)], ident, table)
    with pytest.raises(TypeError, match="uint8"):
        f([frame(image=torch.zeros((64, 96, 3)))], ident, table)
    with pytest.raises(ValueError, match=r"label_image of sample 1 must be \(64, 96, 3\)"):
        f([frame(), frame(label_image=torch.zeros((64, 95, 3), dtype=torch.uint8))], ident, table)
    with pytest.raises(TypeError, match="table"):
        f([frame()], ident, None)
    with pytest.raises(ValueError, match="table"):
        f([frame()], ident, torch.zeros((257, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="table"):
        f([frame()], ident, torch.zeros((7, 4), dtype=torch.uint8))
    with pytest.raises(TypeError, match="points"):
        f([frame(points=np.zeros((5, 3)))], ident, table)
    with pytest.raises(TypeError, match="points"):
        f([frame(points=torch.zeros((5, 3), dtype=torch.float16))], ident, table)
    with pytest.raises(TypeError, match="one dtype per call"):
        f([frame(), frame(points=torch.zeros((5, 3)))], ident, table)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        f([frame(points=torch.zeros((5, 4), dtype=torch.float64))], ident, table)
    with pytest.raises(TypeError, match="row must be float64"):
        f([frame(row=torch.zeros(5))], ident, table)
    with pytest.raises(ValueError, match="col of sample 0"):
        f([frame(col=torch.zeros(4, dtype=torch.float64))], ident, table)
    with pytest.raises(TypeError, match="row of sample 0"):
        f([frame(row=None)], ident, table)
    with pytest.raises(ValueError, match="reflectance"):
        f([frame(reflectance=torch.zeros(5, dtype=torch.uint8)), frame()], ident, table)
    with pytest.raises(TypeError, match="reflectance"):
        f([frame(reflectance=torch.zeros(5, dtype=torch.int64))], ident, table)
    with pytest.raises(ValueError, match="reflectance of sample 0"):
        f([frame(reflectance=torch.zeros(6, dtype=torch.uint8))], ident, table)
    with pytest.raises(ValueError, match="umap.xy"):
        f([frame()], ap.UndistortMap((96, 64), False, torch.zeros((64, 96, 2)), torch.zeros((64, 96), dtype=torch.uint16)), table)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f([frame()], ident, table)                         # well-formed, but on the host

    u = ap.undistort_images
    with pytest.raises(ValueError, match=r"\(B, H, W, 3\)"):
        u(torch.zeros((64, 96, 3), dtype=torch.uint8), ident)
    with pytest.raises(TypeError, match="images"):
        u(None, ident)
    with pytest.raises(ValueError, match="no images"):
        u([], ident)
    with pytest.raises(ValueError, match="image 1"):
        u([torch.zeros((64, 96, 3), dtype=torch.uint8), torch.zeros((64, 96, 1), dtype=torch.uint8)], ident)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        u(torch.zeros((2, 64, 96, 3), dtype=torch.uint8), ident)
