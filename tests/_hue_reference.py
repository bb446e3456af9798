"""numpy restatement of Pillow's RGB <-> HSV conversions of 8-bit images and of torchvision's PIL ``adjust_hue`` on top of them,
the host reference of operation 3 of ``mopa_amd.imageprep`` (``csrc/imageprep.hip``, ``ip_hue``).  ``tests/test_hue_host.py``
holds it against Pillow over all 2^24 colours and all 2^24 HSV triples; ``tests/golden_gen/g14_hue.py`` refuses to write the
fixture unless it agrees.  Also ``ImageEnhance``'s three blends and ``ColorJitter.get_params``, restated for the small cases."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def _clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def rgb_to_hsv(rgb: np.ndarray) -> np.ndarray:
    """(..., 3) uint8 RGB -> (..., 3) uint8 HSV as ``Image.convert("HSV")`` gives it."""
    rgb = np.asarray(rgb, dtype=np.uint8)
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(np.float32)
    s = cr / np.where(grey, 1, maxc).astype(np.float32)                     # float32 quotient
    S = _clip8((s.astype(np.float64) * 255.0).astype(np.int64))
    rc, gc, bc = ((maxc - c).astype(np.float32) / cr for c in (r, g, b))   # float32 quotients
    rc, gc, bc = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc)).astype(np.float32)   # double, stored to float
    x = h.astype(np.float64) / 6.0 + 1.0                                    # in (0, 2): x - floor(x) is fmod(x, 1.0), exactly
    h = (x - np.floor(x)).astype(np.float32)
    H = _clip8((h.astype(np.float64) * 255.0).astype(np.int64))
    return np.stack([np.where(grey, 0, H), np.where(grey, 0, S), maxc], axis=-1).astype(np.uint8)


def _round_away(x):
    """C's ``round``: half away from zero (the arguments here are never negative)."""
    return np.floor(x + 0.5).astype(np.int64)


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    """(..., 3) uint8 HSV -> (..., 3) uint8 RGB as ``Image.convert("RGB")`` of an HSV image gives it."""
    hsv = np.asarray(hsv, dtype=np.uint8)
    H, S, V = (hsv[..., k] for k in range(3))
    h = H.astype(np.float64) * 6.0 / 255.0
    i = np.floor(h)
    f = (h - i).astype(np.float32).astype(np.float64)                       # stored to float
    fs = (S.astype(np.float64) / 255.0).astype(np.float32)                  # stored to float
    v = V.astype(np.float64)
    fsf = (fs * f.astype(np.float32)).astype(np.float64)                    # float * float: a float32 product
    fs = fs.astype(np.float64)
    p = _clip8(_round_away(v * (1.0 - fs)))
    q = _clip8(_round_away(v * (1.0 - fsf)))
    t = _clip8(_round_away(v * (1.0 - fs * (1.0 - f))))
    sel = i.astype(np.int64) % 6
    r = np.choose(sel, [V, q, p, p, t, V])
    g = np.choose(sel, [t, V, V, q, p, p])
    b = np.choose(sel, [p, p, t, V, V, q])
    grey = S == 0
    return np.stack([np.where(grey, V, r), np.where(grey, V, g), np.where(grey, V, b)], axis=-1).astype(np.uint8)


def hue_shift(factor) -> int:
    """``np.int32(hue_factor * 255).astype(np.uint8)`` of ``adjust_hue``: the product in double, truncated toward zero, mod 256.
    ``factor`` is the float32 the draw produced."""
    return int(float(np.float32(factor)) * 255) & 255


def adjust_hue_shift(rgb: np.ndarray, shift: int) -> np.ndarray:
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsv_to_rgb(hsv)


def adjust_hue(rgb: np.ndarray, factor) -> np.ndarray:
    return adjust_hue_shift(rgb, hue_shift(factor))


def all_colours() -> np.ndarray:
    """The 4096 x 4096 x 3 image whose pixel ``n`` (row-major) is (n >> 16, (n >> 8) & 255, n & 255)."""
    n = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(n >> 16) & 255, (n >> 8) & 255, n & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


# ------------------------------------------------------------------------------------------------ ImageEnhance, restated
def _blend(deg, img, f):
    """``Image.blend(degenerate, image, f)`` per channel value: float32, the product rounded before the sum."""
    f = np.float32(f)
    t = deg.astype(np.float32) + (f * (img.astype(np.float32) - deg.astype(np.float32))).astype(np.float32)
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def luma(rgb):
    v = rgb.astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.uint8)


def color_jitter(rgb: np.ndarray, order, factors) -> np.ndarray:
    """The four operations of ``T.ColorJitter`` on an (h, w, 3) uint8 image in the given order."""
    img = np.asarray(rgb, dtype=np.uint8)
    for op, f in zip(order, factors):
        if op == BRIGHTNESS:
            img = _blend(np.zeros_like(img), img, f)
        elif op == CONTRAST:
            L = luma(img)
            mean = int(int(L.sum(dtype=np.int64)) / L.size + 0.5)
            img = _blend(np.full_like(img, mean), img, f)
        elif op == SATURATION:
            img = _blend(np.repeat(luma(img)[..., None], 3, axis=-1), img, f)
        elif op == HUE:
            img = adjust_hue(img, f)
        else:
            raise ValueError(op)
    return img
