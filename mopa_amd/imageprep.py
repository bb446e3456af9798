"""The 2D half of the input pipeline on the device: raw ``uint8`` camera images, SAM masks and float image points of an
iteration -> ``img`` (B,3,h,w) float32, ``sam_mask_ls`` (int32, -100 = ignore) and ``img_indices`` (int64), the 2D side of the
reference's collate layout (``mopa/data/collate.py:125-278``), ready for ``Net2DSeg.forward`` and ``mask_cons_loss``.

Mirrors, bit for bit (fixtures G10 and G14, produced by running Pillow, scipy and the reference's ``refine_sam_mask``), what the datasets do
per sample on the host in ``__getitem__`` (``mopa/data/nuscenes/nuscenes_dataloader.py:347-408``, ``a2d2_dataloader.py:237-263``,
``semantic_kitti_dataloader.py:563-630``):

1. ``resize_bilinear_u8``  ``Image.resize(size, Image.BILINEAR)`` of an 8-bit image -- or, for SemanticKITTI, a crop WINDOW
   ``(left, top, right, bottom)`` that the later stages read through (``image.crop``; no copy is made).
2. ``color_jitter_u8``     ``T.ColorJitter(b, c, s, h)`` on a PIL image = ``ImageEnhance.{Brightness, Contrast, Color}`` and
   ``adjust_hue`` (Pillow's RGB -> HSV, ``H += int(factor * 255)`` modulo 256, HSV -> RGB) in a drawn order.
3. ``to_tensor``           ``np.fliplr``, ``np.array(image, float32) / 255.``, ``(image - mean) / std``, ``np.moveaxis(image, -1, 0)``;
   with ``ori=True`` also the unjittered, unflipped ``/ 255.`` copy (``ori_img`` of ``ema_input``).
4. ``prepare_sam_mask``    ``scipy.ndimage.zoom(mask, 0.25, order=0)`` + ``refine_sam_mask`` (``refine_pseudo_labels.py:72-102``) + crop + flip.
5. ``prepare_img_indices`` the transforms of ``points_img`` (scale with floor, crop origin, ``astype(int64)``, flip).

``prepare_dense_pslabels`` (``csrc/denselabels.hip``, fixture G17) is SemanticKITTI's ``refine_sam_2Dlabels`` for samples with loaded 2D pseudo
labels: ``full_2d_pslabels``, equal to the reference wherever the summed rows decide a mask id.

``prepare_batch`` runs the five stages for the B samples of an iteration with one launch per stage.  The random decisions stay
with the caller (``draw_color_jitter``, ``draw_flip``, ``draw_bottom_crop`` draw them in the reference's order from the reference's
generators); the device part is deterministic.  There is no CPU fallback and -- in the resize form -- no host synchronisation;
the kernels (``csrc/imageprep.hip``) run on the current stream.

Deviations: the datasets' ``assert`` that every index lies inside the image is not made (it would need a
host sync; ``Net2DSeg`` checks the indices it is given).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from ._lib import call, chunk_ranges, host_addr, host_i32, host_ptrs, ptr, query, stream, workspace

MAXB = 32                       # csrc/imageprep.hip IP_MAXB: images per launch
PRECISION_BITS = 22             # Pillow: 32 - 8 - 2
_TILE = 128                     # csrc/imageprep.hip IP_RS_TW
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ host tables
def resize_coeffs(in_size: int, out_size: int) -> np.ndarray:
    """Pillow's coefficients of one BILINEAR pass over an 8-bit image, ``in_size`` -> ``out_size`` samples: int32
    ``(out_size, 2 + ksize)`` rows ``[first source index, count, weights...]``.  The support is ``max(in / out, 1)``; the weights
    are the triangle filter in double, normalised by their sum (added in index order) and rounded to 22-bit fixed point."""
    if in_size < 1 or out_size < 1:
        raise ValueError("resize_coeffs: sizes must be positive")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    k = np.arange(ksize, dtype=np.int64)[None, :]
    x = np.abs((k + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((x < 1.0) & (k < n[:, None]), 1.0 - x, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                      # cumsum adds in index order, like the C loop
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    fixed = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)
    return np.ascontiguousarray(np.concatenate([xmin[:, None].astype(np.int32), n[:, None].astype(np.int32), fixed], axis=1))


def zoom_index(in_size: int, out_size: int) -> np.ndarray:
    """Source index of every output sample of ``scipy.ndimage.zoom(order=0)`` (mode 'constant', grid_mode False), -1 where the
    coordinate ``o * (in - 1) / (out - 1)`` (double) falls outside ``[0, in - 1]`` and the constant 0 is read: for 1208 -> 302
    the last coordinate rounds to just above 1207, so the last row of a zoomed A2D2 mask is all zeros."""
    zoom = (in_size - 1) / (out_size - 1) if out_size > 1 else 1.0
    cc = np.arange(out_size, dtype=np.float64) * zoom
    idx = np.floor(cc + 0.5).astype(np.int64)
    idx[(cc < 0) | (cc > in_size - 1)] = -1
    return idx.astype(np.int32)


def area_min_count(max_area_thre: float, h: int, w: int) -> int:
    """The smallest pixel count refine_sam_mask removes: ``torch.sum(mask) >= max_area_thre * (h * w)`` compares an int64 tensor
    with a Python float, i.e. in float32 (counts below 2^24 are exact there)."""
    if h * w >= 1 << 24:
        raise ValueError("prepare_sam_mask: masks of 2^24 pixels or more are not supported")
    thr = np.float32(max_area_thre * (h * w))
    return int(min(max(math.ceil(float(thr)), -(1 << 30)), 1 << 30)) if np.isfinite(thr) else (1 << 30)


def row_limit(h: int, max_h) -> int:
    """``h_limit`` of ``sam_mask[:h_limit] = -100`` for ``max_h`` (None: no rows are cut)."""
    return 0 if max_h is None else int(h) - int(max_h)


_tables = {}


def _device_table(key, build, dev):
    """Host table -> device, once per key and device, through pinned memory (an asynchronous copy: no host sync)."""
    k = (key, dev.index)
    t = _tables.get(k)
    if t is None:
        pinned = torch.from_numpy(np.ascontiguousarray(build())).pin_memory()
        t = _tables[k] = (pinned.to(dev, non_blocking=True), pinned)
    return t[0]


# ------------------------------------------------------------------------------------------------ draws
def draw_flip(p: float) -> bool:
    """``np.random.rand() < fliplr`` (``nuscenes_dataloader.py:393``, ``semantic_kitti_dataloader.py:607``): one draw from numpy's
    global generator, made even when ``p`` is 0."""
    return bool(np.random.rand() < p)


def draw_bottom_crop(image_size, bottom_crop):
    """SemanticKITTI's crop window ``(left, top, right, bottom)`` (``semantic_kitti_dataloader.py:565-568``): one
    ``np.random.rand()`` for the left edge; ``image_size`` = (W, H), ``bottom_crop`` = (crop_width, crop_height)."""
    left = int(np.random.rand() * (image_size[0] + 1 - bottom_crop[0]))
    return (left, image_size[1] - bottom_crop[1], left + bottom_crop[0], image_size[1])


def _hue_range(hue):
    """torchvision's ``ColorJitter._check_input(hue, "hue", center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)``: the
    ``(lo, hi)`` to draw from, or None when the range is (0, 0) and hue is off.  Every refusal is a ``ValueError`` in
    torchvision's words (torchvision raises ``TypeError`` for a value that is neither a number nor a pair)."""
    if isinstance(hue, (int, float)) and not isinstance(hue, bool):
        if hue < 0:
            raise ValueError("If hue is a single number, it must be non negative.")
        rng = [-float(hue), float(hue)]
    elif isinstance(hue, (tuple, list)) and len(hue) == 2:
        rng = [float(hue[0]), float(hue[1])]
    else:
        raise ValueError("hue should be a single number or a list/tuple with length 2.")
    if not -0.5 <= rng[0] <= rng[1] <= 0.5:
        raise ValueError(f"hue values should be between (-0.5, 0.5), but got {rng}.")
    return None if rng[0] == rng[1] == 0 else tuple(rng)


def hue_shift(factor) -> int:
    """What ``adjust_hue`` adds to H: ``np.int32(hue_factor * 255).astype(np.uint8)`` -- the product in double of the float32
    the draw produced, truncated toward zero, modulo 256."""
    f = float(np.float32(factor))
    if not -0.5 <= f <= 0.5:
        raise ValueError(f"hue_factor ({f}) is not in [-0.5, 0.5].")
    return int(f * 255) & 255


def draw_color_jitter(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.0):
    """The draws of ``torchvision.transforms.ColorJitter(brightness, contrast, saturation, hue)`` for one image, from torch's global
    generator: ``torch.randperm(4)`` for the order of (brightness, contrast, saturation, hue), then one
    ``torch.empty(1).uniform_(max(0, 1 - v), 1 + v)`` per switched-on operation in that fixed order; hue last, from ``(-h, h)`` for
    a float ``0 <= h <= 0.5`` or from a pair inside ``[-0.5, 0.5]`` (anything else is torchvision's ``ValueError``; 0: no draw).
    Returns ``(order, factors)``: the operations in the order they are applied and their factors.

    NOT VERIFIED against torchvision, which is not installed where this was written: ``get_params`` is restated from knowledge
    (DESIGN.md section 4).  The deterministic stages do not depend on it."""
    hue_range = _hue_range(hue)
    perm = torch.randperm(4).tolist()
    factor = {}
    for op, v in ((BRIGHTNESS, brightness), (CONTRAST, contrast), (SATURATION, saturation)):
        if v:
            factor[op] = float(torch.empty(1).uniform_(max(0.0, 1.0 - v), 1.0 + v))
    if hue_range is not None:
        factor[HUE] = float(torch.empty(1).uniform_(hue_range[0], hue_range[1]))
    order = tuple(op for op in perm if op in factor)
    return order, tuple(factor[op] for op in order)


# ------------------------------------------------------------------------------------------------ argument plumbing
def _need_cuda(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"imageprep: {what} must be a torch tensor on the GPU, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"imageprep: {what} must be on the GPU (there is no CPU fallback)")
    return t


def _image_list(images, what="images", channels=3):
    """(B, H, W, 3) tensor or list of (H, W, 3) uint8 tensors -> list of tensors of ONE size (``_on_gpu`` then checks the device)."""
    items = list(images.unbind(0)) if isinstance(images, torch.Tensor) and images.dim() == (4 if channels else 3) else list(images)
    if not items:
        raise ValueError(f"imageprep: no {what}")
    for t in items:                                       # shapes first, so that a malformed call is named as such on any device
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"imageprep: {what} must be torch tensors on the GPU, got {type(t).__name__}")
        ok = t.dim() == 3 and t.shape[2] == channels if channels else t.dim() == 2
        if t.dtype != torch.uint8 or not ok:
            raise ValueError(f"imageprep: {what} must be uint8 {'(H, W, %d)' % channels if channels else '(H, W)'}, "
                             f"got {t.dtype} {tuple(t.shape)}")
        if tuple(t.shape) != tuple(items[0].shape):
            raise ValueError(f"imageprep: all {what} of a call must have one size, got {tuple(items[0].shape)} and {tuple(t.shape)}")
    return items


def _on_gpu(items, what="images"):
    for t in items:
        _need_cuda(t, what)
        if t.device != items[0].device:
            raise ValueError(f"imageprep: all {what} of a call must be on one device")
    return [t.contiguous() for t in items]


def _jitter_tables(jitter, B):
    """list of (order, factors) or None per image -> (int32[B][4], float[B][4], int32[B] hue shifts) host arrays; three times
    None when nothing is on."""
    if jitter is None or all(j is None or len(j[0]) == 0 for j in jitter):
        return None, None, None
    if len(jitter) != B:
        raise ValueError(f"imageprep: {len(jitter)} jitter draws for {B} images")
    order, factor, shift = [-1] * (4 * B), [1.0] * (4 * B), [0] * B
    for b, j in enumerate(jitter):
        if j is None:
            continue
        ops, fs = j
        if len(ops) != len(fs) or len(ops) > 4 or len(set(ops)) != len(ops) or any(o not in (0, 1, 2, 3) for o in ops):
            raise ValueError(f"imageprep: jitter of image {b} must be (order, factors) with each of 0, 1, 2, 3 at most once, got {j!r}")
        for k, (o, f) in enumerate(zip(ops, fs)):
            if o == HUE:
                shift[b] = hue_shift(f)
            elif not (f >= 0):
                raise ValueError(f"imageprep: jitter factor {f!r} of image {b} is negative")
            order[4 * b + k], factor[4 * b + k] = int(o), float(np.float32(f))
    return host_i32(order), (ctypes.c_float * (4 * B))(*factor), host_i32(shift)


def _flags(flip, B):
    if flip is None:
        return None
    flip = [flip] * B if isinstance(flip, (bool, np.bool_)) else list(flip)
    if len(flip) != B:
        raise ValueError(f"imageprep: {len(flip)} flip flags for {B} images")
    return host_i32([1 if f else 0 for f in flip])


def _windows(windows, B, H, W):
    """None or B x (left, top, right, bottom) of ONE size inside the (H, W) image -> (list, oh, ow)."""
    if windows is None:
        return None, H, W
    windows = [tuple(int(v) for v in wd) for wd in windows]
    if len(windows) != B:
        raise ValueError(f"imageprep: {len(windows)} crop windows for {B} images")
    ow, oh = windows[0][2] - windows[0][0], windows[0][3] - windows[0][1]
    for (l, t, r, b) in windows:
        if l < 0 or t < 0 or r > W or b > H or r - l != ow or b - t != oh or ow < 1 or oh < 1:
            raise ValueError(f"imageprep: crop window {(l, t, r, b)} must lie inside the {W}x{H} image and all windows of a call "
                             f"must have one size")
    return windows, oh, ow


# ------------------------------------------------------------------------------------------------ 1. resize
def resize_bilinear_u8(images, size, out=None) -> torch.Tensor:
    """``Image.resize(size, Image.BILINEAR)`` for B 8-bit RGB images of one size: (B, H, W, 3) uint8 (or a list of (H, W, 3))
    -> (B, h, w, 3) uint8, ``size`` = (w, h) as Pillow takes it.  Horizontal pass first, rounded to uint8, then the vertical
    pass on that intermediate; the coefficient tables are built on the host once per (in, out) size and cached on the device."""
    imgs = _on_gpu(_image_list(images))
    B, (H, W, _) = len(imgs), imgs[0].shape
    w, h = int(size[0]), int(size[1])
    dev = imgs[0].device
    xt_host, yt_host = resize_coeffs(W, w), resize_coeffs(H, h)
    xtab = _device_table(("rs", W, w), lambda: xt_host, dev)
    ytab = _device_table(("rs", H, h), lambda: yt_host, dev)
    span = max(int(xt_host[min(x0 + _TILE, w) - 1, 0] + xt_host[min(x0 + _TILE, w) - 1, 1] - xt_host[x0, 0]) for x0 in range(0, w, _TILE))
    if out is None:
        out = torch.empty(B, h, w, 3, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (B, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"resize_bilinear_u8: out must be a contiguous uint8 {(B, h, w, 3)} tensor on {dev}")
    for s, e in chunk_ranges(B, MAXB):
        tab = host_ptrs(imgs[s:e])
        call("mopa_imageprep_resize_u8", host_addr(tab), e - s, H, W, ptr(xtab), xt_host.shape[1] - 2, ptr(ytab), yt_host.shape[1] - 2,
             h, w, span, ptr(out[s:e]), stream())
    return out


# ------------------------------------------------------------------------------------------------ 2 + 3. jitter, to tensor
def _pixels(imgs, windows, jitter, flip, dst_u8, dst_f32, normalizer, ori):
    B, (H, W, _) = len(imgs), imgs[0].shape
    dev = imgs[0].device
    windows, oh, ow = _windows(windows, B, H, W)
    order, factor, shift = _jitter_tables(jitter, B)
    flags = _flags(flip, B)
    norm = None
    if normalizer is not None:
        mean, std = normalizer
        vals = [float(np.float32(v)) for v in list(mean) + list(std)]
        if len(vals) != 6:
            raise ValueError("imageprep: the normaliser is (mean[3], std[3])")
        norm = (ctypes.c_float * 6)(*vals)
    pitch = W * 3
    base = [t.data_ptr() + ((windows[b][1] * W + windows[b][0]) * 3 if windows else 0) for b, t in enumerate(imgs)]
    has_contrast = order is not None and any(order[k] == CONTRAST for k in range(4 * B))
    sums = torch.empty(B, dtype=torch.int64, device=dev) if has_contrast else None
    for s, e in chunk_ranges(B, MAXB):
        tab = host_ptrs(base[s:e])
        o = None if order is None else ctypes.addressof(order) + 16 * s
        f = None if factor is None else ctypes.addressof(factor) + 16 * s
        sh = None if shift is None else ctypes.addressof(shift) + 4 * s
        fl = None if flags is None else ctypes.addressof(flags) + 4 * s
        if has_contrast:
            call("mopa_imageprep_contrast_sums4", host_addr(tab), e - s, pitch, oh, ow, o, f, sh, ptr(sums[s:e]), stream())
        call("mopa_imageprep_pixels4", host_addr(tab), e - s, pitch, oh, ow, o, f, sh, None if sums is None else ptr(sums[s:e]), fl,
             None if dst_u8 is None else ptr(dst_u8[s:e]), None if dst_f32 is None else ptr(dst_f32[s:e]), host_addr(norm),
             None if ori is None else ptr(ori[s:e]), stream())
    return oh, ow


def color_jitter_u8(images, jitter, windows=None) -> torch.Tensor:
    """Brightness / contrast / saturation of ``ImageEnhance`` and torchvision's ``adjust_hue`` on B uint8 images: ``jitter[b]`` =
    ``(order, factors)`` as ``draw_color_jitter`` returns it (operations 0 / 1 / 2 / 3 in the order they are applied, each at
    most once) or None.  The first three are ``Image.blend(degenerate, image, factor)`` in float32: black for brightness, the grey
    image ``L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16`` for saturation, the constant ``int(mean(L) + 0.5)`` of the image
    as it stands in front of the contrast step for contrast (an exact integer reduction).  Hue (factor in [-0.5, 0.5]) is Pillow's
    RGB -> HSV, ``H = (H + hue_shift(factor)) & 255``, HSV -> RGB, made for a zero shift too (the round trip is lossy).
    ``windows``: crop windows read through.  -> (B, h, w, 3) uint8."""
    imgs = _image_list(images)
    B, (H, W, _) = len(imgs), imgs[0].shape
    _, oh, ow = _windows(windows, B, H, W)
    _jitter_tables(jitter, B)
    imgs = _on_gpu(imgs)
    out = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device=imgs[0].device)
    _pixels(imgs, windows, jitter, None, out, None, None, None)
    return out


def _check_batch(out, shape, dev, what):
    if out is None:
        return None
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32:
        raise ValueError(f"imageprep: {what} must be a contiguous float32 {tuple(shape)} tensor, got "
                         f"{getattr(out, 'dtype', type(out).__name__)} {tuple(getattr(out, 'shape', ()))}")
    _need_cuda(out, what)
    if not out.is_contiguous() or (dev is not None and out.device != dev):
        raise ValueError(f"imageprep: {what} must be contiguous and on the images' device")
    return out


def to_tensor(images, out=None, flip=None, normalizer=None, jitter=None, windows=None, ori=False):
    """B uint8 images -> the (B, 3, h, w) float32 batch tensor ``out`` (allocated when None): optional colour jitter (fused, see
    ``color_jitter_u8``), optional left-right flip per image, ``float32(u8) / 255.`` as a true division, optional
    ``(x - mean) / std`` per channel in float32, written CHW.  ``ori=True`` also returns the unjittered, unflipped ``/ 255.``
    copy from the same pass (``ori_img``)."""
    imgs = _image_list(images)
    B, (H, W, _) = len(imgs), imgs[0].shape
    _, oh, ow = _windows(windows, B, H, W)
    _check_batch(out, (B, 3, oh, ow), None, "the batch tensor")
    imgs = _on_gpu(imgs)
    dev = imgs[0].device
    out = _check_batch(out, (B, 3, oh, ow), dev, "the batch tensor")
    if out is None:
        out = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=dev)
    ori_t = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=dev) if ori else None
    _pixels(imgs, windows, jitter, flip, None, out, normalizer, ori_t)
    return (out, ori_t) if ori else out


# ------------------------------------------------------------------------------------------------ 4. SAM mask
def prepare_sam_mask(masks, size=None, max_h=None, row_min=None, max_area_thre=0.1, windows=None, flip=None, out=None) -> torch.Tensor:
    """B SAM masks uint8 (H, W) as the files hold them -> (B, oh, ow) int32 with -100 for ignored pixels, what
    ``refine_sam_mask`` returns and ``mask_cons_loss`` takes.

    ``size`` = (w, h): nearest zoom with ``scipy.ndimage.zoom(order=0)``'s index rule first (None: the mask is used as it is).
    Then ids covering ``>= max_area_thre * h * w`` pixels become -100, and rows ``[: h - max_h]`` -- Python's slice rule, so a
    negative ``h - max_h`` cuts all but the last rows.  ``max_h``: an int or one per image; or ``row_min``: the (B,) int32 device
    tensor ``prepare_img_indices(..., row_min=True)`` reduced from the points (``max_h = h - int(min(points_img[:, 0]))``), read
    by the kernel so that nothing synchronises.  Then the crop ``windows`` (in zoomed coordinates) and the flip."""
    ms = _on_gpu(_image_list(masks, "masks", channels=0), "masks")
    B, (H, W) = len(ms), ms[0].shape
    dev = ms[0].device
    w, h = (W, H) if size is None else (int(size[0]), int(size[1]))
    ytab = None if size is None else _device_table(("zoom", H, h), lambda: zoom_index(H, h), dev)
    xtab = None if size is None else _device_table(("zoom", W, w), lambda: zoom_index(W, w), dev)
    windows, oh, ow = _windows(windows, B, h, w)
    flags = _flags(flip, B)
    mode, limits = 0, None
    if row_min is not None:
        if max_h is not None:
            raise ValueError("prepare_sam_mask: give max_h or row_min, not both")
        _need_cuda(row_min, "row_min")
        if row_min.dtype != torch.int32 or tuple(row_min.shape) != (B,) or not row_min.is_contiguous():
            raise ValueError(f"prepare_sam_mask: row_min must be a contiguous int32 ({B},) tensor")
        mode = 2
    elif max_h is not None:
        mh = [max_h] * B if isinstance(max_h, (int, np.integer)) else list(max_h)
        if len(mh) != B:
            raise ValueError(f"prepare_sam_mask: {len(mh)} max_h values for {B} masks")
        limits = [max(min(row_limit(h, m), (1 << 31) - 1), -(1 << 31)) for m in mh]
        mode = 1
    if out is None:
        out = torch.empty(B, oh, ow, dtype=torch.int32, device=dev)
    elif tuple(out.shape) != (B, oh, ow) or out.dtype != torch.int32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"prepare_sam_mask: out must be a contiguous int32 {(B, oh, ow)} tensor on {dev}")
    min_count = area_min_count(max_area_thre, h, w)
    for s, e in chunk_ranges(B, MAXB):
        tab = host_ptrs(ms[s:e])
        lim = host_i32(limits[s:e]) if mode == 1 else None
        crop = host_i32([v for wd in windows[s:e] for v in (wd[1], wd[0])]) if windows else None
        fl = None if flags is None else ctypes.addressof(flags) + 4 * s
        ws = workspace.get(query("mopa_imageprep_mask_workspace_bytes", e - s), dev)
        call("mopa_imageprep_mask", host_addr(tab), e - s, H, W, ptr(ytab), ptr(xtab), h, w, min_count, mode, host_addr(lim),
             ptr(row_min[s:e]) if mode == 2 else None, host_addr(crop), oh, ow, fl, ptr(out[s:e]), ptr(ws), ws.numel(), stream())
    return out


# ------------------------------------------------------------------------------------------------ 4b. dense pseudo labels
def _per_point(items, B, what, dtype, pts):
    """B (N_b,) tensors of ``dtype``, one value per point of ``pts`` (``_on_gpu`` then checks the device)."""
    items = list(items)
    if len(items) != B:
        raise ValueError(f"prepare_dense_pslabels: {len(items)} {what} arrays for {B} masks")
    for t, p in zip(items, pts):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"prepare_dense_pslabels: {what} must be torch tensors on the GPU, got {type(t).__name__}")
        if t.dtype != dtype or t.dim() != 1 or t.shape[0] != p.shape[0]:
            raise ValueError(f"prepare_dense_pslabels: {what} must be {dtype} ({p.shape[0]},), got {t.dtype} {tuple(t.shape)}")
    return items


def prepare_dense_pslabels(probs, labels, points, masks, num_classes=10, max_area_thre=0.1, windows=None, flip=None, out=None,
                           counts=None) -> torch.Tensor:
    """``full_2d_pslabels`` of B SemanticKITTI target samples: what ``refine_sam_2Dlabels`` returns for the rows that
    ``SemanticKITTISCN.preprocess`` expands (``semantic_kitti_dataloader.py:443-451``), then the crop ``windows`` and the ``flip``
    of ``__getitem__`` -> (B, oh, ow) int32 with -100 for ignored pixels, which ``seg_ce`` takes against the flattened
    ``seg_logit_all``.

    Per sample: ``probs`` (N,) float32, the maximum probability per point; ``labels`` (N,) uint8, the raw pseudo labels;
    ``points`` (N, 2) float [row, col] (``ori_img_points``); ``masks`` (H, W) uint8, the SAM mask as the file holds it (one size
    per call).  The row of a point is ``(1 - p) / (num_classes - 1)`` everywhere and ``p`` at its label; the per-class median
    refinement runs over the rows' maxima; the last point of a pixel wins it; every mask id below ``max_area_thre * H * W`` pixels
    is filled with the first arg-max of its summed winning rows (class 0 without a reliable point), the other pixels keep the
    refined label of their point or -100.  Equal to the reference on every id whose float64 sums decide it.

    ``counts``: an optional (B,) int32 device tensor that receives, per sample, the points that were skipped (outside the image,
    a label ``>= num_classes``, a probability outside [0, 1]; the reference raises on the first two).  No host synchronisation."""
    ms = _image_list(masks, "masks", channels=0)
    B, (H, W) = len(ms), ms[0].shape
    if not isinstance(num_classes, (int, np.integer)) or not 2 <= num_classes <= 32:
        raise ValueError(f"prepare_dense_pslabels: num_classes must be an int in [2, 32], got {num_classes!r}")
    C = int(num_classes)
    points = list(points)
    if len(points) != B:
        raise ValueError(f"prepare_dense_pslabels: {len(points)} point arrays for {B} masks")
    for p in points:
        if not isinstance(p, (np.ndarray, torch.Tensor)):
            raise TypeError(f"prepare_dense_pslabels: points must be torch tensors on the GPU or numpy arrays, got {type(p).__name__}")
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"imageprep: points_img must be (N, 2) [row, col], got {tuple(p.shape)}")
    pr = _per_point(probs, B, "probs", torch.float32, points)
    lb = _per_point(labels, B, "labels", torch.uint8, points)
    windows, oh, ow = _windows(windows, B, H, W)
    flags = _flags(flip, B)
    min_count = area_min_count(max_area_thre, H, W)
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, oh, ow) or out.dtype != torch.int32
                            or not out.is_contiguous()):
        raise ValueError(f"prepare_dense_pslabels: out must be a contiguous int32 {(B, oh, ow)} tensor on the masks' device")
    if counts is not None and (not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (B,) or counts.dtype != torch.int32
                               or not counts.is_contiguous()):
        raise ValueError(f"prepare_dense_pslabels: counts must be a contiguous int32 ({B},) tensor on the masks' device")
    ms = _on_gpu(ms, "masks")
    dev = ms[0].device
    pr, lb = _on_gpu(pr, "probs"), _on_gpu(lb, "labels")
    pts = _points(points)
    for t in pts + pr + lb + [t for t in (out, counts) if t is not None]:
        if _need_cuda(t, "every array").device != dev:
            raise ValueError("prepare_dense_pslabels: every array of a call must be on the masks' device")
    if out is None:
        out = torch.empty(B, oh, ow, dtype=torch.int32, device=dev)
    ns = [int(p.shape[0]) for p in pts]
    for s, e in chunk_ranges(B, MAXB):
        tabs = [host_ptrs(ts[s:e]) for ts in (pr, lb, pts, ms)]
        n_host = host_i32(ns[s:e])
        crop = host_i32([v for wd in windows[s:e] for v in (wd[1], wd[0])]) if windows else None
        fl = None if flags is None else ctypes.addressof(flags) + 4 * s
        ws = workspace.get(query("mopa_denselabels_workspace_bytes", e - s, H, W, sum(ns[s:e]), C), dev)
        call("mopa_denselabels", host_addr(tabs[0]), host_addr(tabs[1]), host_addr(tabs[2]), 0 if pts[0].dtype == torch.float32 else 1,
             host_addr(n_host), host_addr(tabs[3]), e - s, H, W, C, min_count, host_addr(crop), oh, ow, fl, ptr(out[s:e]),
             None if counts is None else ptr(counts[s:e]), ptr(ws), ws.numel(), stream())
    return out


# ------------------------------------------------------------------------------------------------ 5. image indices
def _points(points):
    """list of (N, 2) points -> contiguous float32 / float64 device tensors of one dtype (numpy arrays are uploaded; integer
    arrays go through float64, which is where numpy's promotion of ``float * floor(int array)`` takes them)."""
    out = []
    for p in points:
        if isinstance(p, np.ndarray):
            p = torch.from_numpy(np.ascontiguousarray(p)).to(torch.device("cuda", torch.cuda.current_device()))
        _need_cuda(p, "points_img")
        if p.dim() != 2 or p.shape[1] != 2:
            raise ValueError(f"imageprep: points_img must be (N, 2) [row, col], got {tuple(p.shape)}")
        if p.dtype in (torch.float16, torch.bfloat16):
            raise TypeError("imageprep: points_img in half precision are not supported")
        if not p.dtype.is_floating_point:
            p = p.double()
        out.append(p.contiguous())
    if len({p.dtype for p in out}) > 1:
        raise ValueError("imageprep: the points of one call must have one dtype")
    return out


def prepare_img_indices(points, src_size=None, size=None, windows=None, flip=None, ori=False, row_min=False):
    """The datasets' transforms of ``points_img`` (N, 2) [row, col] for B samples, exactly as they write them.

    Resize form (``src_size`` = (W, H), ``size`` = (w, h); nuScenes, A2D2): ``p[:, 0] = float(h) / H * floor(p[:, 0])``,
    ``p[:, 1] = float(w) / W * floor(p[:, 1])`` in the points' dtype (numpy casts the Python float to float32 against a float32
    array), ``astype(int64)``, then the flip ``w - 1 - col``.  Crop form (``windows`` = (left, top, right, bottom) per sample,
    ``size`` = (w, h) of the window; SemanticKITTI): ``keep`` = inside the window, subtraction of the window's origin, truncation,
    flip.  Without both the points are only truncated (and flipped; then ``size`` is needed).

    Returns a dict: ``img_indices`` (list of (N, 2) int64 -- ALL points, see ``keep``), ``keep`` (crop form: list of (N,) bool),
    ``ori_img_indices`` (``ori=True``: the truncated points before crop and flip), ``row_min`` (``row_min=True``: (B,) int32,
    ``int(min(p[:, 0]))`` of the scaled points, for ``prepare_sam_mask``).  No host synchronisation."""
    pts = _points(points)
    B = len(pts)
    if B == 0:
        raise ValueError("imageprep: no points")
    dev = pts[0].device
    flags = _flags(flip, B)
    if flags is not None and any(flags) and size is None:
        raise ValueError("prepare_img_indices: the flip needs size = (w, h)")
    sy = sx = 1.0
    mode = 1
    if src_size is not None:
        if windows is not None:
            raise ValueError("prepare_img_indices: resize and crop in one call are not a form the datasets have")
        mode = 0
        sy, sx = float(size[1]) / src_size[1], float(size[0]) / src_size[0]
    win = [(0, 0, 0, 0)] * B if windows is None else [tuple(int(v) for v in wd) for wd in windows]
    if len(win) != B:
        raise ValueError(f"imageprep: {len(win)} crop windows for {B} point sets")
    ns = [p.shape[0] for p in pts]
    idx = [torch.empty(n, 2, dtype=torch.int64, device=dev) for n in ns]
    ori_t = [torch.empty(n, 2, dtype=torch.int64, device=dev) for n in ns] if ori else None
    keep = [torch.empty(n, dtype=torch.uint8, device=dev) for n in ns] if windows is not None else None
    rmin = torch.empty(B, dtype=torch.int32, device=dev) if row_min else None
    for s, e in chunk_ranges(B, MAXB):
        tabs = [host_ptrs(ts[s:e]) if ts is not None else None for ts in (pts, idx, ori_t, keep)]
        n_host, w_host = host_i32(ns[s:e]), host_i32([v for wd in win[s:e] for v in wd])
        fl = None if flags is None else ctypes.addressof(flags) + 4 * s
        call("mopa_imageprep_indices", host_addr(tabs[0]), host_addr(n_host), e - s, 0 if pts[0].dtype == torch.float32 else 1, mode, sy, sx,
             host_addr(w_host), 0 if size is None else int(size[0]), fl, host_addr(tabs[1]), host_addr(tabs[2]), host_addr(tabs[3]),
             None if rmin is None else ptr(rmin[s:e]), stream())
    res = {"img_indices": idx}
    if keep is not None:
        res["keep"] = [k.bool() for k in keep]
    if ori:
        res["ori_img_indices"] = ori_t
    if row_min:
        res["row_min"] = rmin
    return res


# ------------------------------------------------------------------------------------------------ the batch
def prepare_batch(samples, out=None, resize=None, normalizer=None, ema_input=False, max_area_thre=0.1, num_classes=10) -> dict:
    """The 2D side of one iteration's batch from the B raw samples, one launch per stage for all of them.

    ``samples``: B dicts with ``image`` (H, W, 3) uint8 and ``points_img`` (N, 2) float (device tensors; images of one size per
    call), optionally ``sam_mask`` (H, W) uint8, and the sample's draws: ``jitter`` = ``draw_color_jitter(...)`` or None, ``flip``
    = ``draw_flip(p)``, ``crop`` = ``draw_bottom_crop(...)`` (SemanticKITTI; all or none of a call), ``max_h`` (an int; default:
    from the points, ``h - int(min(points_img[:, 0]))``, reduced on the device).  ``resize`` = (w, h) as the dataset configs give
    it (nuScenes, A2D2) or None.  ``out``: the (B, 3, h, w) float32 batch tensor to fill (allocated when None).  Samples with a
    ``sam_mask`` may also carry ``probs_2d`` (N,) float32 and ``pseudo_label_2d`` (N,) uint8 (SemanticKITTI's pseudo-label form;
    all or none of a call, not with a resize): the result then has ``full_2d_pslabels`` (list of (h, w) int32 with the crop and
    flip of ``sam_mask_ls``; ``prepare_dense_pslabels`` with ``num_classes``) and nothing else changes.

    Returns ``img`` (B, 3, h, w), ``img_indices`` (list of (N', 2) int64), ``sam_mask_ls`` (list of (h, w) int32; when the samples
    carry masks), with ``ema_input`` ``ori_img`` (list of (3, h', w') float32: the resized -- SemanticKITTI: the uncropped --
    image ``/ 255.``) and ``ori_img_indices``; in the crop form also ``keep`` (list of (N,) bool: which rows of the per-point side
    arrays survive the crop, as ``voxelize_scan`` returns it).

    The resize form makes no host synchronisation.  The crop form compacts the index arrays by their keep masks, which needs ONE
    read-back of the masks per call (like ``voxelize_scan``)."""
    samples = list(samples)
    if not samples:
        raise ValueError("prepare_batch: no samples")
    B = len(samples)
    first = samples[0]["image"]
    if not isinstance(first, torch.Tensor) or first.dim() != 3:
        raise ValueError("prepare_batch: image must be a uint8 (H, W, 3) tensor")
    H, W = int(first.shape[0]), int(first.shape[1])
    crops = [s.get("crop") for s in samples]
    if any(c is not None for c in crops) and not all(c is not None for c in crops):
        raise ValueError("prepare_batch: either every sample of a call has a crop window or none")
    windows = crops if crops[0] is not None else None
    if windows is not None and resize is not None and tuple(resize) != (W, H):
        raise ValueError("prepare_batch: resize and crop in one call are not a form the datasets have")
    do_resize = resize is not None and tuple(resize) != (W, H)
    w, h = (int(resize[0]), int(resize[1])) if do_resize else (W, H)
    has_ps = [s.get("probs_2d") is not None and s.get("pseudo_label_2d") is not None for s in samples]
    if any(s.get("probs_2d") is not None or s.get("pseudo_label_2d") is not None for s in samples) and not all(has_ps):
        raise ValueError("prepare_batch: either every sample of a call has probs_2d and pseudo_label_2d or none")
    if has_ps[0] and (any(s.get("sam_mask") is None for s in samples) or do_resize):
        raise ValueError("prepare_batch: probs_2d / pseudo_label_2d need a sam_mask and no resize (the SemanticKITTI form)")
    win, oh, ow = _windows(windows, B, h, w)
    _check_batch(out, (B, 3, oh, ow), None, "the batch tensor")      # every shape is checked before anything is launched
    imgs = _on_gpu(_image_list([s["image"] for s in samples]))
    dev = imgs[0].device
    jitter = [s.get("jitter") for s in samples]
    flip = [bool(s.get("flip", False)) for s in samples]
    res = {}
    # 1. resize (the datasets skip it when the image already has the size)
    small = list(resize_bilinear_u8(imgs, resize).unbind(0)) if do_resize else imgs
    # 2 + 3. jitter, flip, /255., normalisation
    img = _check_batch(out, (B, 3, oh, ow), dev, "the batch tensor")
    if img is None:
        img = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=dev)
    same_pass = ema_input and win is None
    ori = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=dev) if same_pass else None
    _pixels(small, win, jitter, flip, None, img, normalizer, ori)
    if ema_input and not same_pass:                        # SemanticKITTI keeps the uncropped image (dataloader :559-560)
        ori = torch.empty(B, 3, h, w, dtype=torch.float32, device=dev)
        _pixels(small, None, None, None, None, ori, None, None)
    res["img"] = img
    # 5. indices (before the masks: they may take their row limit from the points)
    has_mask = [s.get("sam_mask") is not None for s in samples]
    if any(has_mask) and not all(has_mask):
        raise ValueError("prepare_batch: either every sample of a call has a sam_mask or none")
    need_min = has_mask[0] and any(s.get("max_h") is None for s in samples)
    if need_min and not all(s.get("max_h") is None for s in samples):
        raise ValueError("prepare_batch: give max_h for every sample of a call or for none")
    ind = prepare_img_indices([s["points_img"] for s in samples], src_size=(W, H) if do_resize else None, size=(ow, oh),
                              windows=win, flip=flip, ori=ema_input, row_min=need_min)
    # 4. masks
    if has_mask[0]:
        masks = prepare_sam_mask([s["sam_mask"] for s in samples], size=(w, h) if do_resize else None,
                                 max_h=None if need_min else [s["max_h"] for s in samples], row_min=ind.get("row_min"),
                                 max_area_thre=max_area_thre, windows=win, flip=flip)
        res["sam_mask_ls"] = list(masks.unbind(0))
    if has_ps[0]:                                          # 4b. dense pseudo labels: the raw points on the unrefined mask
        dense = prepare_dense_pslabels([s["probs_2d"] for s in samples], [s["pseudo_label_2d"] for s in samples],
                                       [s["points_img"] for s in samples], [s["sam_mask"] for s in samples], num_classes=num_classes,
                                       max_area_thre=max_area_thre, windows=win, flip=flip)
        res["full_2d_pslabels"] = list(dense.unbind(0))
    idx = ind["img_indices"]
    if win is not None:
        keep = ind["keep"]
        ns = [k.numel() for k in keep]
        host = torch.cat(keep).cpu().numpy()               # the one read-back of the crop form
        sel = torch.from_numpy(np.flatnonzero(host)).to(dev)
        counts = [int(c.sum()) for c in np.split(host, np.cumsum(ns)[:-1])]
        idx = list(torch.cat(idx).index_select(0, sel).split(counts))
        res["keep"] = keep
    res["img_indices"] = idx
    if ema_input:
        res["ori_img"] = list(ori.unbind(0))
        res["ori_img_indices"] = ind["ori_img_indices"]
    return res
