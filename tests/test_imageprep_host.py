"""The written contract of mopa_amd/imageprep.py against fixture G10 (tests/golden_gen/g10_imageprep.py: Pillow, scipy and the
reference's refine_sam_mask, run on the host), without a GPU: a plain-numpy restatement of the five stages reproduces every fixture
array exactly; imageprep's host tables equal the restatement's; the draw helpers consume the generators as documented; bad
arguments are refused."""
import math
import os

import numpy as np
import pytest
import torch

from mopa_amd import imageprep as ip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_imageprep.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


# ------------------------------------------------------------------------------------------------ the restatement
def np_coeffs(n_in, n_out):
    """One pass of Pillow's 8-bit BILINEAR resize: per output sample (first source index, count, 22-bit weights)."""
    scale = n_in / n_out
    fscale = max(scale, 1.0)
    support = fscale
    rows = []
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        ws, total = [], 0.0
        for x in range(lo, hi):
            t = abs((x - center + 0.5) * (1.0 / fscale))
            wv = 1.0 - t if t < 1.0 else 0.0
            ws.append(wv)
            total += wv
        if total != 0.0:
            ws = [v / total for v in ws]
        rows.append((lo, hi - lo, [int(0.5 + v * (1 << 22)) for v in ws]))
    return rows


def np_resize(img, size):
    w, h = size
    H, W, _ = img.shape
    cx, cy = np_coeffs(W, w), np_coeffs(H, h)
    src = img.astype(np.int64)
    hor = np.empty((H, w, 3), np.int64)
    for x, (lo, n, ws) in enumerate(cx):
        acc = np.full((H, 3), 1 << 21, np.int64)
        for k in range(n):
            acc += ws[k] * src[:, lo + k]
        hor[:, x] = np.clip(acc >> 22, 0, 255)                  # the intermediate is uint8
    out = np.empty((h, w, 3), np.int64)
    for y, (lo, n, ws) in enumerate(cy):
        acc = np.full((w, 3), 1 << 21, np.int64)
        for k in range(n):
            acc += ws[k] * hor[lo + k]
        out[y] = np.clip(acc >> 22, 0, 255)
    return out.astype(np.uint8)


def np_luma(img):
    i = img.astype(np.int64)
    return (19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 0x8000) >> 16


def np_blend(deg, img, f):
    f = np.float32(f)
    d, v = deg.astype(np.float32), img.astype(np.float32)
    t = d + (f * (v - d)).astype(np.float32)                    # float32; the product is rounded before the sum
    t = t.astype(np.float32)
    if 0.0 <= f <= 1.0:
        return t.astype(np.int64).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int64))).astype(np.uint8)


def np_jitter(img, order, factors):
    for op, f in zip(order, factors):
        if op == 0:
            deg = np.zeros_like(img)
        elif op == 1:
            lum = np_luma(img)
            deg = np.full_like(img, int(int(lum.sum()) / lum.size + 0.5))
        else:
            deg = np.repeat(np_luma(img)[..., None], 3, -1).astype(np.uint8)
        img = np_blend(deg, img, f)
    return img


def np_to_tensor(img, flip, norm):
    x = img.astype(np.float32) / np.float32(255.0)
    if flip:
        x = x[:, ::-1]
    if norm is not None:
        x = (x - np.asarray(norm[0], np.float32)) / np.asarray(norm[1], np.float32)
    return np.ascontiguousarray(np.moveaxis(x, -1, 0))


def np_zoom_index(n_in, n_out):
    z = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
    out = []
    for o in range(n_out):
        c = o * z
        out.append(-1 if (c < 0 or c > n_in - 1) else int(math.floor(c + 0.5)))
    return np.asarray(out, np.int32)


def np_mask(src, size, max_h, window, flip, thre=0.1):
    m = src.astype(np.int32)
    if size is not None:
        ys, xs = np_zoom_index(src.shape[0], size[1]), np_zoom_index(src.shape[1], size[0])
        m = np.where((ys[:, None] < 0) | (xs[None, :] < 0), 0, m[np.maximum(ys, 0)][:, np.maximum(xs, 0)])
    h, w = m.shape
    counts = np.bincount(m.reshape(-1), minlength=256)
    big = counts.astype(np.float32) >= np.float32(thre * (h * w))
    out = np.where(big[m], -100, m).astype(np.int32)
    if max_h is not None:
        out[:h - max_h] = -100
    if window is not None:
        left, top, right, bottom = window
        out = out[top:bottom, left:right]
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def np_indices(p, src_size=None, size=None, window=None, flip=False):
    p = p.copy()
    keep = None
    if src_size is not None:
        p[:, 0] = np.asarray(float(size[1]) / src_size[1], p.dtype) * np.floor(p[:, 0])
        p[:, 1] = np.asarray(float(size[0]) / src_size[0], p.dtype) * np.floor(p[:, 1])
    ori = np.trunc(p).astype(np.int64)
    row_min = int(p[:, 0].min())
    if window is not None:
        left, top, right, bottom = window
        keep = (p[:, 0] >= top) & (p[:, 0] < bottom) & (p[:, 1] >= left) & (p[:, 1] < right)
        p = p - np.asarray([top, left], p.dtype)
    idx = np.trunc(p).astype(np.int64)
    if flip:
        idx[:, 1] = size[0] - 1 - idx[:, 1]
    return idx, keep, ori, row_min


# ------------------------------------------------------------------------------------------------ fixture == contract
def test_restatement_reproduces_the_resize_fixtures(g):
    assert int(g["r_n"]) >= 4
    for k in range(int(g["r_n"])):
        assert np.array_equal(np_resize(g[f"r{k}_in"], tuple(g[f"r{k}_size"])), g[f"r{k}_out"]), k


def test_restatement_reproduces_the_jitter_fixtures(g):
    seen = set()
    for k in range(int(g["j_n"])):
        order, fs = tuple(g[f"j{k}_order"]), tuple(g[f"j{k}_factor"])
        seen.add(order)
        got = np_jitter(g["j_img"][int(g[f"j{k}_img"])], order, fs)
        assert np.array_equal(got, g[f"j{k}_out"]), (k, order, fs)
    assert len([o for o in seen if len(o) == 3]) == 6


def test_restatement_reproduces_the_to_tensor_fixtures(g):
    for k in range(4):
        got = np_to_tensor(g["t_in"], bool(g[f"t{k}_flip"]), g["t_norm"] if g[f"t{k}_normalise"] else None)
        assert got.dtype == np.float32 and np.array_equal(got, g[f"t{k}_out"]), k


def _mask_args(g, k):
    size = tuple(int(v) for v in g[f"m{k}_size"])
    window = tuple(int(v) for v in g[f"m{k}_window"])
    max_h = int(g[f"m{k}_max_h"])
    return (g[f"m{k}_in"], None if size[0] < 0 else size, None if max_h == -999999 else max_h, None if window[0] < 0 else window,
            bool(g[f"m{k}_flip"]))


def test_restatement_reproduces_the_mask_fixtures(g):
    for k in range(int(g["m_n"])):
        got = np_mask(*_mask_args(g, k))
        assert np.array_equal(got, g[f"m{k}_out"]), k
    # the pinned quirks: an id AT the threshold goes, one pixel below stays; the last row of the 88 -> 22 zoom reads the constant
    assert (g["m0_out"] == 5).sum() == 0 and (g["m0_out"] == 6).sum() == 55
    assert np_zoom_index(88, 22)[-1] == -1 and np_zoom_index(1208, 302)[-1] == -1 and np_zoom_index(900, 225)[-1] == 899
    assert set(np.unique(g["m1_out"][-1])) <= {0, -100}
    # a negative limit cuts all but the last rows
    k = [k for k in range(int(g["m_n"])) if int(g[f"m{k}_max_h"]) == 25][0]
    assert (g[f"m{k}_out"][:-3] == -100).all() and (g[f"m{k}_out"][-3:] != -100).any()


def _idx_args(g, k):
    form = str(g[f"i{k}_form"])
    if form == "resize":
        return dict(src_size=tuple(g[f"i{k}_src_size"]), size=tuple(g[f"i{k}_size"]), flip=bool(g[f"i{k}_flip"]))
    win = tuple(int(v) for v in g[f"i{k}_window"])
    return dict(window=win, size=(win[2] - win[0], win[3] - win[1]), flip=bool(g[f"i{k}_flip"]))


def test_restatement_reproduces_the_index_fixtures(g):
    dtypes = set()
    for k in range(int(g["i_n"])):
        p = g[f"i{k}_in"]
        dtypes.add(p.dtype)
        idx, keep, ori, row_min = np_indices(p, **_idx_args(g, k))
        if keep is not None:
            assert np.array_equal(keep, g[f"i{k}_keep"]), k
            idx = idx[keep]
        assert np.array_equal(idx, g[f"i{k}_out"]) and np.array_equal(ori, g[f"i{k}_ori"]) and row_min == int(g[f"i{k}_row_min"]), k
    assert dtypes == {np.dtype(np.float32), np.dtype(np.float64)}


# ------------------------------------------------------------------------------------------------ host tables
@pytest.mark.parametrize("n_in,n_out", [(1600, 400), (900, 225), (1920, 480), (1208, 302), (1242, 480), (375, 146), (101, 37), (57, 23),
                                        (40, 40), (80, 13), (7, 1)])
def test_coefficient_tables_equal_the_restatement(n_in, n_out):
    tab = ip.resize_coeffs(n_in, n_out)
    ref = np_coeffs(n_in, n_out)
    assert tab.dtype == np.int32 and tab.shape[0] == n_out
    for o, (lo, n, ws) in enumerate(ref):
        assert tab[o, 0] == lo and tab[o, 1] == n and list(tab[o, 2:2 + n]) == ws and not tab[o, 2 + n:].any(), o


@pytest.mark.parametrize("n_in,n_out", [(88, 22), (120, 30), (1208, 302), (900, 225), (1600, 400), (1920, 480), (57, 23), (33, 9), (5, 1)])
def test_zoom_index_tables_equal_the_restatement(n_in, n_out):
    assert np.array_equal(ip.zoom_index(n_in, n_out), np_zoom_index(n_in, n_out))


def test_area_threshold_and_row_limit():
    assert ip.area_min_count(0.1, 20, 28) == 56
    assert ip.area_min_count(0.1, 20, 30) == 60                 # 0.1 * 600 = 60.00000000000001: compared in float32, like torch
    assert ip.area_min_count(0.1, 225, 400) == 9000
    assert ip.row_limit(22, 15) == 7 and ip.row_limit(22, 25) == -3 and ip.row_limit(22, None) == 0


# ------------------------------------------------------------------------------------------------ draws
def test_draw_helpers_consume_the_generators_as_documented():
    np.random.seed(5)
    a = np.random.rand(3)
    np.random.seed(5)
    assert ip.draw_flip(0.5) == bool(a[0] < 0.5)
    assert ip.draw_bottom_crop((1242, 375), (480, 302)) == (int(a[1] * (1242 + 1 - 480)), 73, int(a[1] * 763) + 480, 375)
    assert ip.draw_flip(0.0) is False and np.random.rand() != a[2]       # the flip draws even when it cannot happen
    torch.manual_seed(7)
    perm = torch.randperm(4).tolist()
    fs = [float(torch.empty(1).uniform_(0.6, 1.4)) for _ in range(3)]
    after = torch.rand(1)
    torch.manual_seed(7)
    order, factors = ip.draw_color_jitter(0.4, 0.4, 0.4)
    assert torch.equal(torch.rand(1), after)
    assert order == tuple(o for o in perm if o != 3) and factors == tuple(fs[o] for o in order)
    assert all(0.6 <= f <= 1.4 for f in factors)
    torch.manual_seed(7)
    order, factors = ip.draw_color_jitter(0.4, 0.0, 0.4)                   # contrast off: no draw for it
    assert 1 not in order and len(factors) == 2


# ------------------------------------------------------------------------------------------------ argument validation
def test_bad_arguments_raise_clear_errors():
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    wide = torch.zeros(8, 12, 3, dtype=torch.uint8)
    pts = torch.zeros(4, 2)
    # CPU tensors: there is no CPU fallback
    with pytest.raises(RuntimeError, match="GPU"):
        ip.prepare_batch([{"image": img, "points_img": pts}])
    with pytest.raises(RuntimeError, match="GPU"):
        ip.resize_bilinear_u8([img], (4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ip.prepare_sam_mask([torch.zeros(8, 8, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="GPU"):
        ip.prepare_img_indices([pts])
    with pytest.raises(TypeError):
        ip.to_tensor([np.zeros((8, 8, 3), np.uint8)])
    # mixed image sizes in one call
    with pytest.raises(ValueError, match="one size"):
        ip.prepare_batch([{"image": img, "points_img": pts}, {"image": wide, "points_img": pts}])
    with pytest.raises(ValueError, match="one size"):
        ip.resize_bilinear_u8([img, wide], (4, 4))
    # a batch tensor of the wrong shape
    with pytest.raises(ValueError, match="batch tensor"):
        ip.prepare_batch([{"image": img, "points_img": pts}], out=torch.zeros(1, 3, 8, 9))
    with pytest.raises(ValueError, match="batch tensor"):
        ip.prepare_batch([{"image": img, "points_img": pts}], resize=(4, 2), out=torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="batch tensor"):
        ip.to_tensor([img], out=torch.zeros(2, 3, 8, 8))
    # a crop window outside the image, a crop for some samples only, not an image
    with pytest.raises(ValueError, match="crop window"):
        ip.to_tensor([img], windows=[(0, 0, 9, 8)])
    with pytest.raises(ValueError, match="every sample"):
        ip.prepare_batch([{"image": img, "points_img": pts, "crop": (0, 0, 4, 4)}, {"image": img, "points_img": pts}])
    with pytest.raises(ValueError, match="uint8"):
        ip.to_tensor([img.float()])
