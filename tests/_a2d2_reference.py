"""The numpy restatement of csrc/a2d2prep.hip: the yardstick of mopa_amd/a2d2prep.py, bit for bit.

OpenCV is not available to this project, so nothing here was produced by or compared with ``cv2.undistort``; the chain is written
from OpenCV's published algorithm (initUndistortRectifyMap into a CV_16SC2 + CV_16UC1 fixed-point map, remap INTER_LINEAR with
BORDER_CONSTANT 0).  The map uses plain elementwise float64 ufuncs, which round once per operation like the kernel's operators (contraction off);
the remap is integer arithmetic.  The cameras below have A2D2's magnitude and are SYNTHETIC (not the dataset's calibration)."""
from fractions import Fraction

import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
DIST_BARREL = (-0.24, -0.33, 0.001, -0.0003, 0.0)
DIST_PINCUSHION = (0.2, 0.05, 0.002, -0.001, 0.01)
DIST_TINY = (0.4, 0.1, 0.01, -0.01, 0.02)
DIST_RATIONAL = (0.2, 0.05, 0.002, -0.001, 0.01, 0.03, -0.02, 0.005)      # k4..k6 non-zero: the denominator is not 1


def camera(W, dist, focal=1.0, lens="Telecam", fx=None, fy=None, c=None):
    """A cams_lidars.json camera entry of A2D2's magnitude scaled to width W (synthetic); K' = K with the focal lengths x focal."""
    s = W / 1920
    fx = 1687.3 * s if fx is None else fx
    fy = 1783.4 * s if fy is None else fy
    cx, cy = (965.4 * s, 684.4 * s) if c is None else c
    return {"CamMatrixOriginal": [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]],
            "CamMatrix": [[fx * focal, 0.0, cx], [0.0, fy * focal, cy], [0.0, 0.0, 1.0]],
            "Distortion": [list(dist)], "Lens": lens}


# name -> (W, H, camera); the cases of tests/test_gpu_a2d2prep.py and the coverage conditions of tests/test_a2d2prep_host.py
CASES = {
    "identity": (64, 48, camera(64, (0.0, 0.0, 0.0, 0.0), fx=50.0, fy=50.0, c=(32.0, 24.0))),
    "barrel": (96, 64, camera(96, DIST_BARREL)),
    "zoom_out": (96, 64, camera(96, DIST_BARREL, 0.6)),
    "odd_pincushion": (67, 45, camera(67, DIST_PINCUSHION, 0.7)),
    "tiny": (33, 17, camera(33, DIST_TINY, 0.5)),
    "rational": (67, 45, camera(67, DIST_RATIONAL, 0.7)),
}
FULL = (1920, 1208, camera(1920, DIST_BARREL))


def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then the one rounding to float64)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fused_columns(cam, W):
    """iu = rint(u * 32) of the columns of a camera WITHOUT distortion as a compiler that contracts u = fx * xd + cx into one fma
    would give them (with zero distortion xd = x exactly, so this is the only place where contraction can show)."""
    K, Kn = cam["CamMatrixOriginal"], cam["CamMatrix"]
    assert not np.any(cam["Distortion"])
    x = (np.arange(W, dtype=np.float64) - Kn[0][2]) / Kn[0][0]
    return fix32(np.array([fma(K[0][0], v, K[0][2]) for v in x]))


def contraction_camera(W=64, H=4, seed=5):
    """A camera without distortion on which the chain rounded once per operation and a contracted chain give DIFFERENT map
    entries, found by search: K' = [[64, 0, 32], [0, 64, 2]] makes x = (j - 32) / 64 exact; for a random fx and column j0, cx is the
    float64 nearest to (k + 1/2) / 32 - fx * x0, so that fx * x0 + cx lies within an ulp of a rounding tie of rint(u * 32): there
    round(round(fx * x0) + cx) and round(fx * x0 + cx) fall on different sides of the tie for about every other draw.
    -> (camera, columns where the two differ)."""
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        fx, j0 = float(rng.uniform(40, 90)), int(rng.integers(0, W))
        x0 = (j0 - 32.0) / 64.0
        tie = Fraction(2 * int(rng.integers(8 * 32, 56 * 32)) + 1, 64)
        cx = float(tie - Fraction(fx) * Fraction(x0))
        cam = {"CamMatrixOriginal": [[fx, 0.0, cx], [0.0, 64.0, 2.0], [0.0, 0.0, 1.0]],
               "CamMatrix": [[64.0, 0.0, 32.0], [0.0, 64.0, 2.0], [0.0, 0.0, 1.0]], "Distortion": [[0.0, 0.0, 0.0, 0.0]], "Lens": "Telecam"}
        xy, frac = undistort_map(cam, (W, H))
        iu = xy[0, :, 0].astype(np.int64) * 32 + (frac[0].astype(np.int64) & 31)
        differ = np.flatnonzero(iu != fused_columns(cam, W))
        if len(differ):
            return cam, differ
    raise AssertionError("no camera found on which contraction shows")


def fix32(u):
    """rint(u * 32) half to even, saturated to int32; non-finite -> INT32_MIN."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = u * 32.0
        fin = np.isfinite(s)
        r = np.clip(np.rint(np.where(fin, s, 0.0)), float(I32_MIN), float(I32_MAX))
    return np.where(fin, r.astype(np.int64), I32_MIN).astype(np.int32)


def undistort_map(cam, size):
    """-> xy (H, W, 2) int16 [sx, sy], frac (H, W) uint16 = fy5 * 32 + fx5."""
    W, H = size
    K, Kn = np.array(cam["CamMatrixOriginal"], np.float64), np.array(cam["CamMatrix"], np.float64)
    d = np.zeros(8)
    dd = np.array(cam["Distortion"], np.float64).reshape(-1)
    d[:len(dd)] = dd
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    with np.errstate(all="ignore"):
        x = (j - Kn[0, 2]) / Kn[0, 0]
        y = (i - Kn[1, 2]) / Kn[1, 1]
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        t = (2.0 * x) * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * t) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * t
        u = fx * xd + cx
        v = fy * yd + cy
    iu, iv = fix32(u), fix32(v)
    xy = np.stack([np.clip(iu >> 5, -32768, 32767), np.clip(iv >> 5, -32768, 32767)], -1).astype(np.int16)
    frac = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return xy, frac


def taps(src, xy):
    """The four taps p00, p01, p10, p11 (H, W, C) int64 of every destination pixel and whether each lies inside the source."""
    H, W = src.shape[:2]
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    out, ins = [], []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        p = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        out.append(np.where(inside[..., None], p, 0))
        ins.append(inside)
    return out, ins


def weights(frac):
    f = frac.astype(np.int64)
    fx, fy = f & 31, f >> 5
    return (32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy


def remap(src, xy, frac):
    """(H, W, 3) uint8 through the map: the closed form, taps outside the source count as 0."""
    (p00, p01, p10, p11), _ = taps(src, xy)
    w00, w01, w10, w11 = (w[..., None] for w in weights(frac))
    return ((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10).astype(np.uint8)


def table_weights():
    """cv2.remap's INTER_LINEAR table for INTER_BITS = 5 as published (initInterTab2D with fixpt: float weights (1-fy)(1-fx) ... x
    32768 rounded with saturate_cast<short>, then the sum forced to 32768 by adding the difference to the largest (or taking it
    from the smallest) weight): (1024, 4) int64 [w00, w01, w10, w11].  At frac = 0 the float weight 1.0 saturates to 32767 and
    the missing 1 lands on the last entry: [32767, 0, 0, 1]."""
    out = np.zeros((1024, 4), np.int64)
    one = np.arange(32, dtype=np.float32) / np.float32(32)
    for fy in range(32):
        for fx in range(32):
            wy = (np.float32(1) - one[fy], one[fy])
            wx = (np.float32(1) - one[fx], one[fx])
            w = np.array([wy[a] * wx[b] for a in (0, 1) for b in (0, 1)], np.float32)
            iw = np.clip(np.rint(w * np.float32(32768)), -32768, 32767).astype(np.int64)
            diff = int(iw.sum()) - 32768
            if diff:
                # the products are exact multiples of 32, so only frac = 0 (32768 saturated to 32767) gets here; the published
                # table has the missing unit on the last entry there
                iw[3] -= diff
            out[fy * 32 + fx] = iw
    return out


def remap_table_form(p, tab_row):
    """(sum w_k p_k + 16384) >> 15: FixedPtCast<int, uchar, 15> of cv2.remap."""
    return (int(np.dot(tab_row, p)) + (1 << 14)) >> 15


def outside(xy, size):
    """-> (wholly, partly): per destination pixel, whether all / some but not all of its four taps lie outside the source."""
    W, H = size
    _, ins = taps(np.zeros((H, W, 1), np.uint8), xy)
    n_in = sum(i.astype(np.int64) for i in ins)
    return n_in == 0, (n_in > 0) & (n_in < 4)


def partly_with_weight_zero(xy, frac, size):
    """Pixels with a tap outside the source whose weight is 0 (the tap cannot matter, whatever the border)."""
    W, H = size
    _, ins = taps(np.zeros((H, W, 1), np.uint8), xy)
    return np.any([(~i) & (w == 0) for i, w in zip(ins, weights(frac))], 0)


def classes(pixels, table):
    """(N, 3) uint8 -> (N,) uint8: the index of the last table row equal to the pixel, else K (preprocess.py:115-120)."""
    out = np.full(len(pixels), len(table), np.int64)
    for k, rgb in enumerate(np.asarray(table)):
        idx = (rgb == pixels).all(1)
        if idx.any():
            out[idx] = k
    return out.astype(np.uint8)


def prepare_frame(label_und, points, row, col, reflectance, table):
    """preprocess.py:96-141 after the undistortion; a point outside the image gets K and is counted.
    -> points, feats, seg_labels, points_img, bad."""
    H, W = label_und.shape[:2]
    r, c = row.astype(np.int32), col.astype(np.int32)
    ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
    seg = np.full(len(r), len(table), np.int64).astype(np.uint8)
    seg[ok] = classes(label_und[r[ok], c[ok], :], table)
    feats = reflectance / 255 if reflectance is not None else np.ones((points.shape[0], 1))
    return (points.astype(np.float32), feats.astype(np.float32), seg, np.stack([row, col], 1).astype(np.float32), int((~ok).sum()))


# The colour table of the label tests: K = 7 rows, six colours; row 6 repeats row 1, so the last equal row (6) must win and class 1
# never appears.  Row 0 is black, the border value: a pixel wholly outside the source is a real class.
TABLE = np.array([[0, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 255, 0]], np.uint8)
FOREIGN = (9, 9, 9)            # a colour that is in no row


def block_labels(W, H):
    """The label image of the tests: blocks of 32 x 16 pixels in the six colours of TABLE, and an 8 x 8 patch of FOREIGN in the
    middle.  Undistorted, the blended block borders and the patch are in no row of the table (class K)."""
    by, bx = np.arange(H)[:, None] // 16, np.arange(W)[None, :] // 32
    im = TABLE[:6][(by * 3 + bx * 2 + 1) % 6].copy()
    im[H // 2 - 4:H // 2 + 4, W // 2 - 4:W // 2 + 4] = FOREIGN
    return np.ascontiguousarray(im)


def lidar_points(rng, n, W, H, n_bad=0):
    """n points of a frame: float64 xyz, row / col with fractional parts inside the image (the last n_bad of them outside: one row
    below 0, one column at W), reflectance 0..255."""
    pts = rng.normal(0, 20, (n, 3))
    row, col = rng.uniform(0, H, n), rng.uniform(0, W, n)
    if n_bad:
        row[-n_bad::2] = -1.5
        col[-n_bad + 1::2] = W + 0.25
    return pts, row, col, rng.integers(0, 256, n).astype(np.uint8)


# a seventh small case: zero distortion, built so that a contracted (fma) chain gives other map entries than the stated one
CONTRACT_CAMERA, CONTRACT_COLUMNS = contraction_camera()
CASES["contract"] = (64, 4, CONTRACT_CAMERA)
