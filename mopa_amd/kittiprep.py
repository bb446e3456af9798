"""SemanticKITTI's on-the-fly projection on the device: the raw scans of an iteration (the ``.bin`` and ``.label`` contents as
loaded, the calibration's ``proj_matrix``, optionally PatchWork++'s ground index list) -> what ``data_extraction`` + ``preprocess``
(``mopa/data/semantic_kitti/semantic_kitti_dataloader.py:349-371,422-507``) leave in ``data_dict``: the front-half points that fall
into the camera image, their remission, labels and image coordinates, and the keep mask over the z-filtered scan.  The outputs are
the inputs of ``imageprep.prepare_batch`` (``points_img``, crop form) and ``scanprep.prepare_batch_3d`` (``points``, ``seg_labels``).

Mirrors, bit for bit (fixture G13, produced by running the reference's ``preprocess`` and ``select_points_in_frustum``): the
``z > -3`` filter, ``label & 0xFFFF`` and ``astype(np.int16)``, the ground mask, ``x > 0``, the float32 product with
``proj_matrix``, the perspective divide, ``np.around(., 2)``, the strict frustum test, the boolean compaction of every per-point
array and the ``fliplr``.  ``prepare_scans_kitti`` runs this for the B samples with a fixed number of launches
(``csrc/kittiprep.hip``: every kernel covers all scans) and exactly ONE blocking read-back, of the 2 B counts that size the
outputs.  There is no CPU fallback.

The product: each row is the fused chain ``fma(m3, 1, fma(m2, z, fma(m1, y, m0 * x)))``, which is what
numpy's float32 ``matmul`` computed, bit for bit, on the host the fixture was generated on.  Another BLAS may order or fuse the sum
differently; the fixture's generator asserts the equality and fails where it does not hold.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from ._lib import call, chunk_ranges, host_addr, host_i32, host_ptrs, ptr, query, stream
from ._prep import check_devices, ground_mask, image_size_wh, out_rows, read_counts, tensor_checker

_NAME = "prepare_scans_kitti"
_PSEUDO = ("ori_keep_idx", "ori_img_points")
_OPTIONAL = ("g_indices",) + _PSEUDO


# ------------------------------------------------------------------------------------------------ argument checks
def _check(samples, image_size):
    """Types, dtypes and shapes first (so that a malformed call is named as such on any device), then the device."""
    if not samples:
        raise ValueError(f"{_NAME}: no samples")
    w, h = image_size_wh(_NAME, image_size)
    for key in _OPTIONAL:
        have = [s.get(key) is not None for s in samples]
        if any(have) and not all(have):
            raise ValueError(f"{_NAME}: either every sample of a call has `{key}` or none")
    first = samples[0]
    if (first.get("ori_keep_idx") is None) != (first.get("ori_img_points") is None):
        raise ValueError(f"{_NAME}: `ori_keep_idx` and `ori_img_points` come together")
    pseudo = first.get("ori_keep_idx") is not None
    tensor, tensors = tensor_checker(_NAME)
    for b, s in enumerate(samples):
        scan = tensor(b, s, "scan", (torch.float32,), "float32")
        if scan.dim() != 2 or scan.shape[1] != 4:
            raise ValueError(f"{_NAME}: scan of sample {b} must be (N, 4), got {tuple(scan.shape)}")
        n = scan.shape[0]
        label = tensor(b, s, "label", (torch.int32, torch.int64), "int32 (the uint32 file viewed as int32) or int64")
        if tuple(label.shape) != (n,):
            raise ValueError(f"{_NAME}: label of sample {b} must be ({n},) for {n} points, got {tuple(label.shape)}")
        if label.dtype != first["label"].dtype:
            raise TypeError(f"{_NAME}: label must have one dtype per call")
        if not pseudo:
            m = s.get("proj_matrix")
            if not isinstance(m, np.ndarray):
                raise TypeError(f"{_NAME}: proj_matrix of sample {b} must be a numpy array on the host, got {type(m).__name__}")
            if m.shape != (3, 4) or m.dtype.kind != "f":
                raise ValueError(f"{_NAME}: proj_matrix of sample {b} must be a (3, 4) float array, got {m.shape} {m.dtype}")
        if s.get("g_indices") is not None:
            g = tensor(b, s, "g_indices", (torch.int32,), "int32")
            if g.dim() != 1:
                raise ValueError(f"{_NAME}: g_indices of sample {b} must be (G,), got {tuple(g.shape)}")
        if pseudo:
            k = tensor(b, s, "ori_keep_idx", (torch.bool,), "bool")
            if k.dim() != 1:
                raise ValueError(f"{_NAME}: ori_keep_idx of sample {b} must be (Nz,), got {tuple(k.shape)}")
            p = tensor(b, s, "ori_img_points", (torch.float32,), "float32")
            if p.dim() != 2 or p.shape[1] != 2:
                raise ValueError(f"{_NAME}: ori_img_points of sample {b} must be (Nk, 2), got {tuple(p.shape)}")
    check_devices(_NAME, tensors)
    return w, h, pseudo


# ------------------------------------------------------------------------------------------------ the batch
def prepare_scans_kitti(samples, image_size, with_full: bool = False) -> dict:
    """``data_extraction`` + ``preprocess`` for the B scans of one iteration, every stage as one launch for all of them.

    ``samples``: B dicts of device tensors holding the file contents as loaded: ``scan`` (N, 4) float32 (the ``.bin``), ``label``
    (N,) int32 (the uint32 ``.label`` viewed as int32) or int64, ``proj_matrix`` (3, 4) float on the HOST (numpy; cast to float32
    as the reference does), optionally ``g_indices`` (G,) int32 (PatchWork++'s index list into the raw scan; all samples or none).
    The pseudo-label form (``:430-469``; all samples or none) has ``ori_keep_idx`` (Nz,) bool and ``ori_img_points`` (Nk, 2)
    float32 as loaded: nothing is projected, the given mask is the keep mask and the given image points are handed through.
    ``image_size`` = (W, H), as PIL's ``.size``.

    Returns lists of B device tensors: ``points`` (Nk, 3) float32, ``feats`` (Nk, 1) float32, ``seg_labels`` (Nk,) int16 (the low
    16 bits, wrapping as ``astype(np.int16)``), ``points_img`` (Nk, 2) float32 ``[row, col]``, ``ori_keep_idx`` (Nz,) bool in the
    numbering of the z-filtered scan, ``g_indices`` (Nk,) bool when given; with ``with_full`` ``full_scan`` (Nz, 3) float32 and
    ``all_seg_labels`` (Nz,) int16 (the z-filtered scan); and ``counts``, a (B, 2) int64 numpy array ``[Nz, Nk]`` on the host.

    One blocking read-back per call (the counts).  What only the counts can tell is refused after it: a ground index outside its
    scan (IndexError, as numpy raises), a loaded mask or loaded image points of another length than the scan gives (ValueError)."""
    samples = list(samples)
    w, h, pseudo = _check(samples, image_size)
    B = len(samples)
    dev = samples[0]["scan"].device
    has_g = samples[0].get("g_indices") is not None
    scans = [s["scan"].contiguous() for s in samples]
    scans = [t if t.data_ptr() % 16 == 0 else t.clone() for t in scans]          # the kernels load a row as one 16-byte word
    labels = [s["label"].contiguous() for s in samples]
    ns = [t.shape[0] for t in scans]
    label_i64 = int(labels[0].dtype == torch.int64)
    rows = query("mopa_kittiprep_rows_per_block")

    chunks = []
    for s, e in chunk_ranges(B, query("mopa_kittiprep_max_scans")):
        Bc = e - s
        c = {"s": s, "e": e, "B": Bc, "scan": host_ptrs(scans[s:e]), "label": host_ptrs(labels[s:e]), "n": host_i32(ns[s:e]),
             "proj": None, "gmask": None, "bad": None}
        total = sum(ns[s:e])
        nblk = sum(-(-n // rows) for n in ns[s:e])
        c["ws"] = torch.empty(query("mopa_kittiprep_workspace_bytes", nblk), dtype=torch.uint8, device=dev)
        c["flags"] = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        c["counts"] = torch.empty(2 * Bc + 1, dtype=torch.int64, device=dev)
        mask_t = mask_n = None
        if pseudo:
            c["hold"] = [samples[b]["ori_keep_idx"].contiguous() for b in range(s, e)]
            mask_t, mask_n = host_ptrs(c["hold"]), host_i32([t.numel() for t in c["hold"]])
        else:
            m = np.stack([samples[b]["proj_matrix"].astype(np.float32) for b in range(s, e)]).reshape(-1)
            c["proj"] = (ctypes.c_float * (12 * Bc))(*m.tolist())
        if has_g:
            c["gmask"], c["bad"] = ground_mask(call, [samples[b]["g_indices"] for b in range(s, e)], c["n"])
        call("mopa_kittiprep_count", host_addr(c["scan"]), host_addr(c["n"]), host_addr(c["proj"]), host_addr(mask_t), host_addr(mask_n),
             Bc, w, h, ptr(c["flags"]), ptr(c["bad"]), ptr(c["counts"]), ptr(c["ws"]), c["ws"].numel(), stream())
        chunks.append(c)

    # the one read-back: per chunk [Nz, Nk] of every scan, then the number of ground indices outside their scan
    counts = read_counts(_NAME, chunks, 2)
    nz, nk = [int(v) for v in counts[:, 0]], [int(v) for v in counts[:, 1]]
    if pseudo:
        for b, s in enumerate(samples):
            if s["ori_keep_idx"].numel() != nz[b]:
                raise ValueError(f"{_NAME}: ori_keep_idx of sample {b} has {s['ori_keep_idx'].numel()} entries, its scan has {nz[b]} points with z > -3")
            if s["ori_img_points"].shape[0] != nk[b]:
                raise ValueError(f"{_NAME}: ori_img_points of sample {b} has {s['ori_img_points'].shape[0]} rows, ori_keep_idx keeps {nk[b]} points")
    Z, K = sum(nz), sum(nk)

    _rows = functools.partial(out_rows, device=dev)
    none = (None, 0, None)
    out = {"points": _rows(K, 3), "feats": _rows(K, 1), "seg": _rows(K, dtype=torch.int16), "img": none if pseudo else _rows(K, 2),
           "keep": _rows(Z, dtype=torch.uint8), "g": _rows(K, dtype=torch.uint8) if has_g else none,
           "full": _rows(Z, 3) if with_full else none, "all_seg": _rows(Z, dtype=torch.int16) if with_full else none}
    z0 = k0 = 0
    for c in chunks:
        s, e = c["s"], c["e"]
        at = {k: None if addr is None else addr + (z0 if k in ("keep", "full", "all_seg") else k0) * step for k, (_, step, addr) in out.items()}
        call("mopa_kittiprep_scatter", host_addr(c["scan"]), host_addr(c["label"]), label_i64, host_addr(c["n"]), host_addr(c["proj"]), c["B"],
             w, h, ptr(c["flags"]), ptr(c["gmask"]), at["points"], at["feats"], at["seg"], at["img"], at["keep"], at["g"], at["full"],
             at["all_seg"], ptr(c["ws"]), c["ws"].numel(), stream())
        z0 += sum(nz[s:e])
        k0 += sum(nk[s:e])
    points, feats, seg, img, keep, g_out, full, all_seg = (out[k][0] for k in ("points", "feats", "seg", "img", "keep", "g", "full", "all_seg"))

    res = {"points": list(points.split(nk)), "feats": list(feats.split(nk)), "seg_labels": list(seg.split(nk)),
           "points_img": [s["ori_img_points"] for s in samples] if pseudo else list(img.split(nk)),
           "ori_keep_idx": list(keep.view(torch.bool).split(nz)), "counts": counts}
    if has_g:
        res["g_indices"] = list(g_out.view(torch.bool).split(nk))
    if with_full:
        res["full_scan"], res["all_seg_labels"] = list(full.split(nz)), list(all_seg.split(nz))
    return res
