"""A2D2's offline preprocessing of a frame on the device: the camera image and the colour-coded label image as decoded, the
lidar ``points`` / ``row`` / ``col`` / ``reflectance`` of the frame's ``.npz`` as loaded -> what ``DummyDataset.__getitem__``
(``mopa/data/a2d2/preprocess.py:96-141`` with ``undistort_image``, ``:26-44``) leaves in the pickle and in the saved image: the
undistorted image, ``points`` and ``feats`` as float32, ``points_img`` ``[row, col]`` and the class index of every point read from
the undistorted label image.  The outputs are the inputs of ``imageprep.prepare_batch`` (``img``, ``points_img``; resize form) and
``scanprep.prepare_batch_3d`` (``points``, ``seg_labels``).

``undistort_map`` builds the inverse map of a camera once (``csrc/a2d2prep.hip``); ``prepare_frames_a2d2`` then makes two launches
for any B up to 32 frames (the remap of all planes, the points of all frames; larger batches are walked in chunks of 64 planes and
32 frames) and no read-back.  There is no CPU fallback.  PNG decoding, file
I/O, the npz, the fisheye cameras, frames without ``row`` and the pickle stay with the caller.

Arithmetic: the map is the stated float64 chain, every operation rounded once, stored in OpenCV's
``CV_16SC2`` + ``CV_16UC1`` fixed-point layout; the remap is the integer closed form of ``cv2.remap(INTER_LINEAR)``'s weight table
with a constant 0 border.  The yardstick is the numpy restatement ``tests/_a2d2_reference.py``, bit for bit; OpenCV was not at
hand: UNVERIFIED against ``cv2.undistort`` itself.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import torch

from ._lib import call, chunk_ranges, host_addr, host_i32, host_ptrs, ptr, query, stream

_NAME = "a2d2prep"
DIST_LENGTHS = (4, 5, 8)       # k1, k2, p1, p2[, k3[, k4, k5, k6]]
_REFL = {torch.uint8: 1, torch.float32: 2, torch.float64: 3}


@dataclass
class UndistortMap:
    """The inverse map of one camera at one image size.  ``identity``: the camera is not undistorted (``xy`` / ``frac`` are None)."""
    size: tuple                         # (W, H)
    identity: bool
    xy: torch.Tensor | None = None      # (H, W, 2) int16 [sx, sy]: the source pixel of the top-left tap
    frac: torch.Tensor | None = None    # (H, W) uint16 = fy5 * 32 + fx5: the 1/32-pixel fractions


# ------------------------------------------------------------------------------------------------ host helpers
def _size(size, who):
    try:
        w, h = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: size must be (W, H), got {size!r}") from None
    if w < 1 or h < 1 or w > 32767 or h > 32767:
        raise ValueError(f"{who}: size must be (W, H) with sides in 1..32767, got {size!r}")
    return w, h


def camera_params(camera) -> np.ndarray:
    """The 16 float64 the map kernel takes from a ``cams_lidars.json`` camera entry: [fx, fy, cx, cy] of ``CamMatrixOriginal``,
    the same of ``CamMatrix``, then k1, k2, p1, p2, k3, k4, k5, k6 (absent coefficients 0)."""
    who = f"{_NAME}.undistort_map"
    if not isinstance(camera, dict):
        raise TypeError(f"{who}: camera must be the dict of cams_lidars.json, got {type(camera).__name__}")
    out = []
    for key in ("CamMatrixOriginal", "CamMatrix"):
        if key not in camera:
            raise ValueError(f"{who}: camera lacks `{key}`")
        try:
            m = np.array(camera[key], dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError(f"{who}: camera[{key!r}] must be 3 x 3 numbers") from None
        if m.shape != (3, 3) or not np.isfinite(m).all():
            raise ValueError(f"{who}: camera[{key!r}] must be a finite (3, 3) matrix, got shape {m.shape}")
        if m[0, 1] != 0 or m[1, 0] != 0 or m[2].tolist() != [0.0, 0.0, 1.0]:
            raise ValueError(f"{who}: camera[{key!r}] must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew)")
        if m[0, 0] == 0 or m[1, 1] == 0:
            raise ValueError(f"{who}: camera[{key!r}] has a zero focal length")
        out += [m[0, 0], m[1, 1], m[0, 2], m[1, 2]]
    if "Distortion" not in camera:
        raise ValueError(f"{who}: camera lacks `Distortion`")
    try:
        d = np.array(camera["Distortion"], dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError(f"{who}: camera['Distortion'] must be numbers") from None
    if len(d) not in DIST_LENGTHS:
        raise ValueError(f"{who}: camera['Distortion'] must hold {', '.join(map(str, DIST_LENGTHS[:-1]))} or {DIST_LENGTHS[-1]} coefficients, got {len(d)}")
    if not np.isfinite(d).all():
        raise ValueError(f"{who}: camera['Distortion'] is not finite")
    return np.concatenate([out, d, np.zeros(8 - len(d))])


def undistort_map(camera, size, device=None) -> UndistortMap:
    """The map ``cv2.undistort(image, CamMatrixOriginal, Distortion, newCameraMatrix=CamMatrix)`` walks, for images of
    ``size`` = (W, H).  ``camera``: the ``cams_lidars.json`` entry as loaded.  ``Lens == 'Telecam'`` builds the map (one launch;
    keep it: it depends on the camera only); ``'Fisheye'`` is refused (``preprocess.py`` only ever processes ``front_center``, a
    Telecam); any other lens is the pass-through ``undistort_image`` takes (``.identity``, no launch)."""
    who = f"{_NAME}.undistort_map"
    if not isinstance(camera, dict):
        raise TypeError(f"{who}: camera must be the dict of cams_lidars.json, got {type(camera).__name__}")
    w, h = _size(size, who)
    lens = camera.get("Lens")
    if lens == "Fisheye":
        raise NotImplementedError(f"{who}: Lens 'Fisheye' (cv2.fisheye.undistortImage) is not implemented")
    if lens != "Telecam":
        return UndistortMap((w, h), True)
    cam = camera_params(camera)
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the map is built on the GPU (there is no CPU fallback), got device {dev}")
    with torch.cuda.device(dev):
        xy = torch.empty((h, w, 2), dtype=torch.int16, device=dev)
        frac = torch.empty((h, w), dtype=torch.uint16, device=dev)
        call("mopa_a2d2prep_map", cam.ctypes.data, w, h, ptr(xy), ptr(frac), stream())
    return UndistortMap((w, h), False, xy, frac)


def color_table(class_list) -> torch.Tensor:
    """(K, 3) uint8 host tensor of the RGB codes of ``class_list.json`` (``{"#rrggbb": name}``) in file order: row k is the colour of
    class index k (``preprocess.py:61-71``)."""
    who = f"{_NAME}.color_table"
    if not isinstance(class_list, dict) or not class_list:
        raise TypeError(f"{who}: class_list must be the non-empty dict of class_list.json, got {type(class_list).__name__}")
    rows = []
    for k in class_list:
        hx = k.lstrip("#") if isinstance(k, str) else ""
        try:
            if len(hx) != 6:
                raise ValueError
            rows.append([int(hx[i:i + 2], 16) for i in (0, 2, 4)])
        except ValueError:
            raise ValueError(f"{who}: key {k!r} is not '#rrggbb'") from None
    if len(rows) > 256:
        raise ValueError(f"{who}: at most 256 classes, got {len(rows)}")
    return torch.tensor(rows, dtype=torch.uint8)


# ------------------------------------------------------------------------------------------------ argument checks
def _check(who, umap, planes, table=None, samples=None):
    """Types, dtypes and shapes first (so that a malformed call is named as such on any device), then the device.
    planes: [(name, tensor)] of (H, W, 3) uint8.  -> the device."""
    if not isinstance(umap, UndistortMap):
        raise TypeError(f"{who}: umap must be an UndistortMap (undistort_map), got {type(umap).__name__}")
    w, h = umap.size
    tensors = []
    if not umap.identity:
        for name, t, shape, dt in (("umap.xy", umap.xy, (h, w, 2), torch.int16), ("umap.frac", umap.frac, (h, w), torch.uint16)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{who}: {name} must be a contiguous {shape} {dt} tensor")
            tensors.append((name, t))
    if not planes:
        raise ValueError(f"{who}: no images")
    for name, t in planes:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a torch tensor on the GPU, got {type(t).__name__}")
        if t.dtype != torch.uint8:
            raise TypeError(f"{who}: {name} must be uint8, got {t.dtype}")
        if tuple(t.shape) != (h, w, 3):
            raise ValueError(f"{who}: {name} must be ({h}, {w}, 3) for the map's size {w} x {h}, got {tuple(t.shape)}")
        tensors.append((name, t))
    if table is not None or samples is not None:
        if not isinstance(table, torch.Tensor):
            raise TypeError(f"{who}: table must be a torch tensor (color_table(...).cuda()), got {type(table).__name__}")
        if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != 3 or not 1 <= table.shape[0] <= 256:
            raise ValueError(f"{who}: table must be (K, 3) uint8 with 1 <= K <= 256, got {tuple(table.shape)} {table.dtype}")
        tensors.append(("table", table))
        have = [s.get("reflectance") is not None for s in samples]
        if any(have) and not all(have):
            raise ValueError(f"{who}: either every sample of a call has `reflectance` or none")
        for b, s in enumerate(samples):
            p = s.get("points")
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"{who}: points of sample {b} must be a torch tensor on the GPU, got {type(p).__name__}")
            if p.dtype not in (torch.float64, torch.float32):
                raise TypeError(f"{who}: points must be float64 or float32, got {p.dtype}")
            if p.dtype != samples[0]["points"].dtype:
                raise TypeError(f"{who}: points of sample {b} are {p.dtype}, those of sample 0 {samples[0]['points'].dtype}; one dtype per call")
            if p.dim() != 2 or p.shape[1] != 3:
                raise ValueError(f"{who}: points of sample {b} must be (N, 3), got {tuple(p.shape)}")
            n = p.shape[0]
            tensors.append(("points", p))
            for key in ("row", "col"):
                t = s.get(key)
                if not isinstance(t, torch.Tensor):
                    raise TypeError(f"{who}: {key} of sample {b} must be a torch tensor on the GPU, got {type(t).__name__}")
                if t.dtype != torch.float64:
                    raise TypeError(f"{who}: {key} must be float64 (as in the npz), got {t.dtype}")
                if tuple(t.shape) != (n,):
                    raise ValueError(f"{who}: {key} of sample {b} must be ({n},) for {n} points, got {tuple(t.shape)}")
                tensors.append((key, t))
            if have[0]:
                t = s["reflectance"]
                if not isinstance(t, torch.Tensor):
                    raise TypeError(f"{who}: reflectance of sample {b} must be a torch tensor on the GPU, got {type(t).__name__}")
                if t.dtype not in _REFL:
                    raise TypeError(f"{who}: reflectance must be uint8, float32 or float64, got {t.dtype}")
                if t.dtype != samples[0]["reflectance"].dtype:
                    raise TypeError(f"{who}: reflectance of sample {b} is {t.dtype}, that of sample 0 {samples[0]['reflectance'].dtype}; one dtype per call")
                if tuple(t.shape) != (n,):
                    raise ValueError(f"{who}: reflectance of sample {b} must be ({n},) for {n} points, got {tuple(t.shape)}")
                tensors.append(("reflectance", t))
    for name, t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be on the GPU (there is no CPU fallback)")
        if t.device != tensors[0][1].device:
            raise ValueError(f"{who}: {name} is on {t.device}; all tensors of a call must be on one device")
    return tensors[0][1].device


def _as_planes(images, who, name):
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError(f"{who}: {name} must be (B, H, W, 3) or a list of (H, W, 3), got {tuple(images.shape)}")
        return [images[b] for b in range(images.shape[0])]
    if not isinstance(images, (list, tuple)):
        raise TypeError(f"{who}: {name} must be a (B, H, W, 3) tensor or a list of (H, W, 3) tensors, got {type(images).__name__}")
    return list(images)


def _overlap(a, b):
    """Whether the storage ranges of two contiguous tensors overlap."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _remap(umap, srcs, dsts):
    """One launch per mopa_a2d2prep_max_planes() planes: one launch up to 64 planes.  A plane that is not contiguous is copied
    first (one more launch of torch's per such plane); decoded images are contiguous."""
    w, h = umap.size
    srcs = [t.contiguous() for t in srcs]
    for s, e in chunk_ranges(len(srcs), query("mopa_a2d2prep_max_planes")):
        sp, dp = host_ptrs(srcs[s:e]), host_ptrs(dsts[s:e])
        call("mopa_a2d2prep_remap", host_addr(sp), host_addr(dp), e - s, h, w, ptr(umap.xy), ptr(umap.frac), stream())


# ------------------------------------------------------------------------------------------------ images
def undistort_images(images, umap, out=None) -> torch.Tensor:
    """``cv2.undistort`` of B images through the camera's map in one launch.  ``images``: (B, H, W, 3) uint8 device tensor or a list
    of (H, W, 3); up to 64 images are one launch, more are walked in chunks of 64, and an image that is not contiguous is copied
    first.  Returns (B, H, W, 3) uint8 (``out`` if given: contiguous; an ``out`` that overlaps an image is refused, because the
    kernel gathers from the sources while it writes).  With a pass-through map the images are returned as they are (stacked), as
    ``undistort_image`` does."""
    who = f"{_NAME}.undistort_images"
    planes = _as_planes(images, who, "images")
    dev = _check(who, umap, [(f"image {b}", t) for b, t in enumerate(planes)])
    w, h = umap.size
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (len(planes), h, w, 3) or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"{who}: out must be a contiguous ({len(planes)}, {h}, {w}, 3) uint8 tensor on {dev}")
        for b, t in enumerate(planes):
            if _overlap(out, t.contiguous()):
                raise ValueError(f"{who}: out overlaps image {b}; the remap cannot run in place")
    if umap.identity:
        res = images if isinstance(images, torch.Tensor) else torch.stack(planes)
        if out is None:
            return res
        out.copy_(res)
        return out
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((len(planes), h, w, 3), dtype=torch.uint8, device=dev)
        _remap(umap, planes, [out[b] for b in range(len(planes))])
    return out


# ------------------------------------------------------------------------------------------------ the frames
def prepare_frames_a2d2(samples, umap, table, with_label_image=False) -> dict:
    """``DummyDataset.__getitem__`` (``preprocess.py:96-141``) for the B frames of one call: two launches for any B up to 32 (the remap
    of all planes, the points of all frames; chunks of 64 planes / 32 frames beyond that), no read-back.

    ``samples``: B dicts of device tensors.  ``image`` and ``label_image`` (H, W, 3) uint8 as decoded; ``points`` (N, 3) float64 or
    float32; ``row`` and ``col`` (N,) float64; optionally, for all samples or none, ``reflectance`` (N,) uint8, float32 or float64.
    N = 0 is legal.  ``umap``: the camera's ``undistort_map``.  ``table``: ``color_table(class_list)`` on the device, K rows.

    Returns ``img`` (B, H, W, 3) uint8, the undistorted images; lists of B device tensors ``points`` (N, 3) float32, ``feats``
    float32 ((N,) = reflectance / 255, or ones of shape (N, 1) without reflectance: the reference's shapes), ``seg_labels`` (N,)
    uint8 (the index of the LAST table row equal to the undistorted label pixel at ``[int32(row), int32(col)]``, else K; with K =
    256 the reference's uint8 cast wraps K to 0, and so does this), ``points_img`` (N, 2) float32 ``[row, col]``; ``bad_index``
    (B,) int32 on the device: per frame the points whose ``[row, col]`` lies outside the image (the reference would raise or wrap;
    here they get K).  ``MOPA_VALIDATE_LABELS=1`` reads that counter back and raises IndexError naming the frame.  With
    ``with_label_image`` also ``label_img`` (B, H, W, 3) uint8, the undistorted label planes (the same launch)."""
    who = f"{_NAME}.prepare_frames_a2d2"
    samples = list(samples)
    if not samples:
        raise ValueError(f"{who}: no samples")
    for s in samples:
        if not isinstance(s, dict):
            raise TypeError(f"{who}: every sample must be a dict, got {type(s).__name__}")
    planes = [(f"image of sample {b}", s.get("image")) for b, s in enumerate(samples)]
    planes += [(f"label_image of sample {b}", s.get("label_image")) for b, s in enumerate(samples)]
    dev = _check(who, umap, planes, table, samples)
    B = len(samples)
    w, h = umap.size
    K = table.shape[0]
    images = [s["image"] for s in samples]
    labels = [s["label_image"].contiguous() for s in samples]
    with torch.cuda.device(dev):
        res = {}
        if umap.identity:
            res["img"] = torch.stack(images)
            if with_label_image:
                res["label_img"] = torch.stack(labels)
        else:
            res["img"] = torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev)
            srcs, dsts = images, [res["img"][b] for b in range(B)]
            if with_label_image:
                res["label_img"] = torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev)
                srcs, dsts = srcs + labels, dsts + [res["label_img"][b] for b in range(B)]
            _remap(umap, srcs, dsts)

        pts = [s["points"].contiguous() for s in samples]
        rows = [s["row"].contiguous() for s in samples]
        cols = [s["col"].contiguous() for s in samples]
        refl = [s["reflectance"].contiguous() for s in samples] if samples[0].get("reflectance") is not None else None
        kind = _REFL[refl[0].dtype] if refl else 0
        ns = [t.shape[0] for t in pts]
        N = sum(ns)
        table = table.contiguous()
        points = torch.empty((max(N, 1), 3), dtype=torch.float32, device=dev)[:N]      # never a null address
        feats = torch.empty(max(N, 1), dtype=torch.float32, device=dev)[:N]
        seg = torch.empty(max(N, 1), dtype=torch.uint8, device=dev)[:N]
        pimg = torch.empty((max(N, 1), 2), dtype=torch.float32, device=dev)[:N]
        bad = torch.empty(B, dtype=torch.int32, device=dev)
        n0 = 0
        for s, e in chunk_ranges(B, query("mopa_a2d2prep_max_frames")):                  # one launch up to 32 frames
            hp, hr, hc, hl = host_ptrs(pts[s:e]), host_ptrs(rows[s:e]), host_ptrs(cols[s:e]), host_ptrs(labels[s:e])
            hf = host_ptrs(refl[s:e]) if refl else None
            hn = host_i32(ns[s:e])
            call("mopa_a2d2prep_points", host_addr(hp), host_addr(hr), host_addr(hc), host_addr(hf), host_addr(hl), host_addr(hn), e - s,
                 int(pts[0].dtype == torch.float64), kind, ptr(umap.xy), ptr(umap.frac), w, h, ptr(table), K,
                 points.data_ptr() + 12 * n0, feats.data_ptr() + 4 * n0, seg.data_ptr() + n0, pimg.data_ptr() + 8 * n0, ptr(bad, s), stream())
            n0 += sum(ns[s:e])
    res["points"] = list(points.split(ns))
    res["feats"] = [f if refl else f.view(-1, 1) for f in feats.split(ns)]
    res["seg_labels"] = list(seg.split(ns))
    res["points_img"] = list(pimg.split(ns))
    res["bad_index"] = bad
    if os.environ.get("MOPA_VALIDATE_LABELS") == "1":
        got = bad.cpu().tolist()
        for b, v in enumerate(got):
            if v:
                raise IndexError(f"{who}: {v} points of sample {b} have [row, col] outside the {w} x {h} image")
    return res
