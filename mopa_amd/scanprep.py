"""The 3D half of the input pipeline on the device: the raw scans of an iteration (points in metres, raw labels, image indices,
loaded pseudo labels) -> ``x = [locs, feats]``, ``seg_label``, ``img_indices``, ``aug_points_ls``, the pseudo labels and the
bookkeeping masks of the reference's collate layout (``mopa/data/collate.py:182-264``), ready for ``Net3DSeg.forward``.

Mirrors, bit for bit (fixture G11, produced by running the reference's ``augment_and_scale_3d``, ``refine_pseudo_labels`` and
``collate_scn_base``), what the datasets do per sample on the host in ``__getitem__``
(``mopa/data/nuscenes/nuscenes_dataloader.py:339-340,410-465``, ``semantic_kitti_dataloader.py:583-585,632-676``,
``a2d2_dataloader.py:278-315``): rotation, ``round(p * scale) - min``, the random translation, the int64 cast and the in-field
filter ``idxs``; ``seg_label = label_mapping[seg_label][idxs]``, ``img_indices[idxs]``, ``refine_pseudo_labels(...)[idxs]``; the
un-augmented copy for the EMA teacher.  ``prepare_batch_3d`` runs this for the B samples with a fixed number of launches
(``csrc/scanprep.hip``: every kernel covers all scans) and at most ONE read-back: none with ``assume_inside=True`` and no crop
mask, otherwise one blocking copy of the per-scan row counts.  The coordinates are the bits of ``voxelize.rotate_points`` +
``voxelize.voxelize_scan`` per scan.  The random decisions stay with the caller (``draw_augmentation_3d`` draws them in the
reference's order from numpy's global generator).  There is no CPU fallback.

Deviations: ``feats`` has one row per kept point (nuScenes' has one per loaded point; ``Net3DSeg`` ignores the
rest); pseudo labels and ``ori_locs`` are int64 (reference: int32, float32 with integral values); a scan with no points, or whose
``keep_in`` is all false, contributes no rows (the reference raises on the empty ``min``); with ``assume_inside`` nothing is
filtered: a coordinate outside the field is emitted, counted in ``n_outside``, and refused by ``Geometry3D`` at the next forward.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from ._lib import call, chunk_ranges, host_addr, host_i32, host_ptrs, ptr, query, stream, workspace
from ._prep import out_rows
from .voxelize import draw_rotation

MAXB = 32                       # csrc/scanprep.hip SP_MAXB: scans per launch
_LABEL_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3}
_PER_POINT = ("keep_in", "seg_label", "img_indices", "pseudo_label_2d", "probs_2d", "pseudo_label_3d", "probs_3d")


def draw_augmentation_3d(noisy_rot=0.0, flip_x=0.0, flip_y=0.0, rot_z=0.0, transl=False):
    """The draws of ``augment_and_scale_3d`` (``augmentation_3d.py:26-58``) for one scan, from numpy's global generator in the
    reference's order: ``randn(3, 3)``, ``randint(0, 2)`` for flip_x, ``randint(0, 2)`` for flip_y, ``rand()`` for rot_z, then
    ``rand(3)`` for the translation.  -> ``(rot, transl_u)``: the 3x3 float32 matrix (None when no option is on) and the three
    float64 draws (None without translation)."""
    rot = draw_rotation(noisy_rot, flip_x, flip_y, rot_z)
    return rot, (np.random.rand(3) if transl else None)


def take(batch: dict, per_point: torch.Tensor) -> torch.Tensor:
    """Compact any further per-point array -- one row per point of the concatenated input scans -- the way the batch was
    compacted (``[keep_idx][idxs]`` per scan in the reference, ``train_xmuda_mopa.py:314-332``), without a host round trip."""
    return per_point.index_select(0, batch["gather"])


# ------------------------------------------------------------------------------------------------ argument checks
def _check_samples(samples, label_mapping):
    """Types, dtypes and lengths first (so that a malformed call is named as such on any device), then the device."""
    if not samples:
        raise ValueError("prepare_batch_3d: no samples")
    for key in _PER_POINT:
        have = [s.get(key) is not None for s in samples]
        if any(have) and not all(have):
            raise ValueError(f"prepare_batch_3d: either every sample of a call has `{key}` or none")
    tensors = []
    for b, s in enumerate(samples):
        p = s.get("points")
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"prepare_batch_3d: points of sample {b} must be a torch tensor on the GPU, got {type(p).__name__}")
        if p.dtype != torch.float32:
            raise TypeError(f"prepare_batch_3d: points must be float32, got {p.dtype}")
        if p.dim() != 2 or p.shape[1] != 3:
            raise ValueError(f"prepare_batch_3d: points must be (N, 3), got {tuple(p.shape)}")
        n = p.shape[0]
        tensors.append(("points", p))
        for key in _PER_POINT:
            t = s.get(key)
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"prepare_batch_3d: {key} of sample {b} must be a torch tensor on the GPU, got {type(t).__name__}")
            if key == "keep_in":
                ok = t.dtype == torch.bool
            elif key.startswith("probs"):
                ok = t.dtype == torch.float32
            elif key == "img_indices":
                ok = t.dtype == torch.int64
            else:
                ok = t.dtype in _LABEL_DTYPES
            if not ok:
                raise TypeError(f"prepare_batch_3d: {key} has dtype {t.dtype}")
            shape = (n, 2) if key == "img_indices" else (n,)
            if tuple(t.shape) != shape:
                raise ValueError(f"prepare_batch_3d: {key} of sample {b} must be {shape} for {n} points, got {tuple(t.shape)}")
            tensors.append((key, t))
        for key in ("seg_label", "pseudo_label_2d", "pseudo_label_3d"):
            if s.get(key) is not None and s[key].dtype != samples[0][key].dtype:
                raise TypeError(f"prepare_batch_3d: {key} must have one dtype per call")
        for a, c in (("pseudo_label_2d", "probs_2d"), ("pseudo_label_3d", "probs_3d")):
            if (s.get(a) is None) != (s.get(c) is None):
                raise ValueError(f"prepare_batch_3d: `{a}` and `{c}` come together")
        rot, u = s.get("rot"), s.get("transl_u")
        if rot is not None and np.asarray(rot).shape != (3, 3):
            raise ValueError(f"prepare_batch_3d: rot must be 3x3, got {np.asarray(rot).shape}")
        if u is not None and np.asarray(u).shape != (3,):
            raise ValueError(f"prepare_batch_3d: transl_u must hold 3 draws, got {np.asarray(u).shape}")
    if label_mapping is not None:
        if not isinstance(label_mapping, torch.Tensor) or label_mapping.dtype != torch.int64 or label_mapping.dim() != 1 \
                or label_mapping.numel() == 0:
            raise TypeError("prepare_batch_3d: label_mapping must be a 1-D int64 tensor on the GPU")
        tensors.append(("label_mapping", label_mapping))
    for key, t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"prepare_batch_3d: {key} must be on the GPU (there is no CPU fallback)")
        if t.device != tensors[0][1].device:
            raise ValueError("prepare_batch_3d: all tensors of a call must be on one device")


def _upload_i64(values, dev):
    """A few host integers -> device, asynchronously (no host synchronisation that torch would have to make)."""
    return torch.tensor(values, dtype=torch.int64).to(dev, non_blocking=True)


# ------------------------------------------------------------------------------------------------ segmented refinement
def refine_pseudo_labels_segmented(probs, pseudo_labels, ignore_label: int = -100, num_classes=None, out=None):
    """``pseudo.refine_pseudo_labels`` for S independent (probs, labels) pairs in one set of launches: per pair and class, labels
    whose probability is below ``min(lower median, 0.9)`` become ``ignore_label``.  ``probs``: list of (n_s,) float32 (or None: the
    labels are only cast), ``pseudo_labels``: list of (n_s,) integer tensors of one dtype.  -> list of (n_s,) int64 (views of
    ``out``, a (sum n_s,) int64 tensor, when given).  Equal to S separate calls of ``pseudo.refine_pseudo_labels``."""
    labels = [t.contiguous() for t in pseudo_labels]
    if not labels:
        return []
    if any(not t.is_cuda for t in labels):
        raise RuntimeError("refine_pseudo_labels_segmented: the labels must be on the GPU (there is no CPU fallback)")
    if labels[0].dtype not in _LABEL_DTYPES or any(t.dtype != labels[0].dtype for t in labels):
        raise TypeError("refine_pseudo_labels_segmented: the labels must be uint8 / int16 / int32 / int64, one dtype per call")
    ps = None
    if probs is not None:
        if len(probs) != len(labels):
            raise ValueError("refine_pseudo_labels_segmented: one probability array per label array")
        ps = [p.contiguous() for p in probs]
        for p, t in zip(ps, labels):
            if p.dtype != torch.float32 or p.shape != t.shape or p.device != t.device:
                raise ValueError("refine_pseudo_labels_segmented: probs must be float32 of the labels' shape and device")
    dev = labels[0].device
    ns = [t.numel() for t in labels]
    if out is None:
        out = torch.empty(sum(ns), dtype=torch.int64, device=dev)
    outs = list(out.split(ns))
    for s, e in chunk_ranges(len(labels), 2 * MAXB):
        _refine_into(None if ps is None else ps[s:e], labels[s:e], outs[s:e], ignore_label, num_classes, dev)
    return outs


# ------------------------------------------------------------------------------------------------ the batch
def prepare_batch_3d(samples, scale, full_scale: int = 4096, label_mapping=None, refine: bool = True, ema_input: bool = False,
                     assume_inside: bool = False, ignore_label: int = -100, num_classes=None) -> dict:
    """The 3D side of one iteration's batch from the B raw samples, every stage as one launch for all of them.

    ``samples``: B dicts of device tensors: ``points`` (N, 3) float32 in metres; the sample's draws ``rot`` (3x3 float32 or None)
    and ``transl_u`` (3 float64 or None) as ``draw_augmentation_3d`` returns them; optionally ``keep_in`` (N,) bool (SemanticKITTI's
    crop mask: rows with False are removed BEFORE the minimum is taken), ``seg_label`` (N,) uint8 / int16 / int32 / int64 raw ids
    (``label_mapping``, a 1-D int64 device tensor, is applied first; an id outside the table maps to ``ignore_label`` and is
    checked, with a host sync, only under ``MOPA_VALIDATE_LABELS=1``), ``img_indices`` (N, 2) int64 (all points' indices as
    ``imageprep`` returns them un-compacted), ``pseudo_label_2d`` / ``probs_2d`` / ``pseudo_label_3d`` / ``probs_3d`` (N,): with
    ``refine`` each pair is refined per scan over all N points (before ``keep_in``, as the datasets do), then compacted.

    Returns (device tensors; the names are the collate function's): ``x = [locs (M, 4) int64 [x, y, z, b], feats (M, 1) ones]``;
    ``seg_label`` (M,) int64; ``img_indices`` / ``aug_points_ls``: lists of B (M_b, 2) int64 / (M_b, 3) float32 (the rotated points
    of the kept rows); ``pseudo_label_2d`` / ``pseudo_label_3d`` (M,) int64 and ``ori_pslabel_ls`` (list of (N_b,), refined, not
    compacted); ``orig_seg_label`` (list, mapped, compacted by ``keep_in`` only) and ``orig_points_idx`` (list of bool: the
    reference's ``idxs``); ``gather`` (M,) int64 (for every output row the index of its point in the concatenation of the input
    scans, see ``take``), ``offsets`` (B + 1,) int64, ``n_outside`` (int32 scalar).  With ``ema_input``: ``ori_x = [ori_locs,
    ori_feats]`` from the points as loaded (no rotation, no translation, before ``keep_in``, its own field filter), ``ori_keep_idx``
    (list: ``keep_in`` or all true) and ``ori_idxs`` (= ``orig_points_idx``, as the reference stores it).

    ``assume_inside=True`` without ``keep_in``: nothing is removed and NOTHING synchronises with the host; inputs that need no work
    are handed through (``img_indices``, un-rotated ``aug_points_ls``).  Otherwise exactly one read-back per call."""
    samples = list(samples)
    _check_samples(samples, label_mapping)
    B = len(samples)
    dev = samples[0]["points"].device
    scale, full_scale = float(scale), int(full_scale)
    if full_scale <= 0:
        raise ValueError("prepare_batch_3d: full_scale must be positive")
    first = samples[0]
    has = {k: first.get(k) is not None for k in _PER_POINT}
    general = has["keep_in"] or not assume_inside
    pts = [s["points"].contiguous() for s in samples]
    side = {k: [s[k].contiguous() for s in samples] if has[k] else None for k in _PER_POINT}
    ns = [p.shape[0] for p in pts]
    row0 = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    total = int(row0[-1])
    if has["seg_label"] and label_mapping is not None and os.environ.get("MOPA_VALIDATE_LABELS", "0") == "1":
        for b, t in enumerate(side["seg_label"]):
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= label_mapping.numel()):
                raise IndexError(f"prepare_batch_3d: seg_label of sample {b} has ids outside the label mapping")
    res = {}

    # 5. pseudo labels: refined per scan over all its points (flat buffers in the numbering of the concatenated scans)
    ps_flat = {}
    ps_keys = [k for k in ("pseudo_label_2d", "pseudo_label_3d") if has[k]]
    if ps_keys:
        for k in ps_keys:
            ps_flat[k] = torch.empty(total, dtype=torch.int64, device=dev)
        groups = [ps_keys] if len({side[k][0].dtype for k in ps_keys}) == 1 else [[k] for k in ps_keys]
        for g in groups:
            for s, e in chunk_ranges(B, MAXB):
                labs = [t for k in g for t in side[k][s:e]]
                prs = [t for k in g for t in side["probs" + k[-3:]][s:e]] if refine else None
                views = [v for k in g for v in ps_flat[k][row0[s]:row0[e]].split(ns[s:e])]
                _refine_into(prs, labs, views, ignore_label, num_classes, dev)

    # 1. rotation: one buffer for the scans that have a matrix; the others are read through
    rot_ids = [b for b, s in enumerate(samples) if s.get("rot") is not None and ns[b] > 0]
    src = list(pts)
    if rot_ids:
        buf = torch.empty(sum(ns[b] for b in rot_ids), 3, dtype=torch.float32, device=dev)
        for b, v in zip(rot_ids, buf.split([ns[b] for b in rot_ids])):
            src[b] = v
        for s, e in chunk_ranges(len(rot_ids), MAXB):
            ids = rot_ids[s:e]
            r = np.ascontiguousarray(np.stack([np.asarray(samples[b]["rot"], np.float32) for b in ids]))
            st, dt, nt = host_ptrs([pts[b] for b in ids]), host_ptrs([src[b] for b in ids]), host_i32([ns[b] for b in ids])
            call("mopa_scanprep_rotate", host_addr(st), host_addr(dt), host_addr(nt), r.ctypes.data, len(ids), stream())

    # 2 + 3. min / max, keep flags, ordered counts -> offsets
    rows = query("mopa_scanprep_rows_per_block")
    n_outside = torch.zeros((), dtype=torch.int32, device=dev)
    chunks = []
    for s, e in chunk_ranges(B, MAXB):
        Bc = e - s
        seg_src = src[s:e] + (pts[s:e] if ema_input else [])
        seg_n = ns[s:e] * (2 if ema_input else 1)
        seg_keep = (side["keep_in"][s:e] + [None] * (Bc if ema_input else 0)) if has["keep_in"] else None
        S = len(seg_src)
        u = [float(v) for b in range(s, e) for v in (samples[b]["transl_u"] if samples[b].get("transl_u") is not None else (0., 0., 0.))]
        c = {"S": S, "B": Bc, "s": s, "e": e, "src": host_ptrs(seg_src), "keep": host_ptrs(seg_keep) if seg_keep else None,
             "n": host_i32(seg_n), "u": (ctypes.c_double * (3 * Bc))(*u),
             "on": host_i32([samples[b].get("transl_u") is not None for b in range(s, e)]), "hold": (seg_src, seg_keep)}
        nblk = sum(-(-n // rows) for n in seg_n)
        c["ws"] = torch.empty(query("mopa_scanprep_workspace_bytes", nblk), dtype=torch.uint8, device=dev)
        c["flags"] = torch.empty(sum(seg_n), dtype=torch.uint8, device=dev) if general else None
        c["offsets"] = torch.empty(S + 1 + Bc + 1, dtype=torch.int64, device=dev) if general else None
        call("mopa_scanprep_count", host_addr(c["src"]), host_addr(c["keep"]), host_addr(c["n"]), host_addr(c["u"]), host_addr(c["on"]),
             S, Bc, scale, full_scale, int(general), ptr(c["flags"]), ptr(c["offsets"]), ptr(c["ws"]), c["ws"].numel(), stream())
        chunks.append(c)

    # the one read-back: per chunk [first output row of every segment ..., first keep_in row of every scan ...]
    if general:
        dev_off = chunks[0]["offsets"] if len(chunks) == 1 else torch.cat([c["offsets"] for c in chunks])
        host = dev_off.cpu().numpy()
        at = 0
        for c in chunks:
            c["off"] = host[at:at + c["S"] + 1]
            c["koff"] = host[at + c["S"] + 1:at + c["S"] + 1 + c["B"] + 1]
            at += c["S"] + 1 + c["B"] + 1
    else:
        for c in chunks:
            c["off"] = np.concatenate([[0], np.cumsum(list(c["n"]))]).astype(np.int64)
            c["koff"] = c["off"][:c["B"] + 1]
    counts, kcounts, ocounts = [], [], []
    for c in chunks:
        o, Bc = c["off"], c["B"]
        counts += [int(v) for v in np.diff(o[:Bc + 1])]
        kcounts += [int(v) for v in np.diff(c["koff"])]
        ocounts += [int(v) for v in np.diff(o[Bc:])]
    M, K, Mo = sum(counts), sum(kcounts), sum(ocounts)

    # 4. compaction
    def _rows(n, *shape, dtype=torch.int64):               # (address, tensor)
        t, _, addr = out_rows(n, *shape, dtype=dtype, device=dev)
        return addr, t

    (locs_p, locs), (gather_p, gather) = _rows(M, 4), _rows(M)
    ori_p, ori_locs = _rows(Mo, 4) if ema_input else (None, None)
    mask1_p, mask1 = _rows(K, dtype=torch.uint8) if has["keep_in"] else (None, None)
    gather1_p, gather1 = _rows(K) if has["keep_in"] else (None, None)
    m0 = k0 = o0 = 0
    for c in chunks:
        s, e, Bc = c["s"], c["e"], c["B"]
        call("mopa_scanprep_compact", host_addr(c["src"]), host_addr(c["keep"]), host_addr(c["n"]), host_addr(c["u"]), host_addr(c["on"]),
             c["S"], Bc, s, scale, full_scale, int(not general), ptr(c["flags"]), locs_p + 32 * m0,
             None if ori_p is None else ori_p + 32 * o0, gather_p + 8 * m0, int(row0[s]), None if mask1_p is None else mask1_p + k0,
             None if gather1_p is None else gather1_p + 8 * k0, ptr(n_outside), ptr(c["ws"]), c["ws"].numel(), stream())
        c["m0"], c["k0"] = m0, k0
        m0 += int(c["off"][Bc])
        k0 += int(c["koff"][Bc])
        o0 += int(c["off"][c["S"]] - c["off"][Bc])

    # side arrays through the gather
    through = not general                                   # nothing was removed: inputs that need no work are handed through
    lab_dt = _LABEL_DTYPES[side["seg_label"][0].dtype] if has["seg_label"] else 0
    seg_out = torch.empty(M, dtype=torch.int64, device=dev) if has["seg_label"] else None
    orig_out = None
    if has["seg_label"] and general:
        orig_out = torch.empty(K if has["keep_in"] else total, dtype=torch.int64, device=dev)
    img_out = torch.empty(M, 2, dtype=torch.int64, device=dev) if has["img_indices"] and not through else None
    pts_out = torch.empty(M, 3, dtype=torch.float32, device=dev) if not through else None
    ps_out = {k: torch.empty(M, dtype=torch.int64, device=dev) for k in ps_keys} if not through else {}
    for c in chunks:
        s, e, Bc = c["s"], c["e"], c["B"]
        nt = host_i32(ns[s:e])
        lt = host_ptrs(side["seg_label"][s:e]) if has["seg_label"] else None
        it = host_ptrs(side["img_indices"][s:e]) if has["img_indices"] else None
        st = host_ptrs(src[s:e])
        Mc, Kc, m0, k0, r0 = int(c["off"][Bc]), int(c["koff"][Bc]), c["m0"], c["k0"], int(row0[s])
        ps2, ps3 = ps_flat.get("pseudo_label_2d"), ps_flat.get("pseudo_label_3d")
        if through:
            if has["seg_label"]:
                call("mopa_scanprep_take", None, 0, Mc, host_addr(nt), Bc, host_addr(lt), lab_dt, ptr(label_mapping),
                     0 if label_mapping is None else label_mapping.numel(), int(ignore_label), None, None, None, None,
                     seg_out.data_ptr() + 8 * m0, None, None, None, None, stream())
            continue
        call("mopa_scanprep_take", gather_p + 8 * m0, r0, Mc, host_addr(nt), Bc, host_addr(lt), lab_dt, ptr(label_mapping),
             0 if label_mapping is None else label_mapping.numel(), int(ignore_label), host_addr(it), host_addr(st),
             None if ps2 is None else ps2.data_ptr() + 8 * r0, None if ps3 is None else ps3.data_ptr() + 8 * r0,
             None if seg_out is None else seg_out.data_ptr() + 8 * m0, None if img_out is None else img_out.data_ptr() + 16 * m0,
             pts_out.data_ptr() + 12 * m0, None if ps2 is None else ps_out["pseudo_label_2d"].data_ptr() + 8 * m0,
             None if ps3 is None else ps_out["pseudo_label_3d"].data_ptr() + 8 * m0, stream())
        if orig_out is not None:                            # the mapped labels before the field filter (after keep_in)
            if has["keep_in"]:
                call("mopa_scanprep_take", gather1_p + 8 * k0, r0, Kc, host_addr(nt), Bc, host_addr(lt), lab_dt, ptr(label_mapping),
                     0 if label_mapping is None else label_mapping.numel(), int(ignore_label), None, None, None, None,
                     orig_out.data_ptr() + 8 * k0, None, None, None, None, stream())
            else:
                call("mopa_scanprep_take", None, 0, int(row0[e] - r0), host_addr(nt), Bc, host_addr(lt), lab_dt, ptr(label_mapping),
                     0 if label_mapping is None else label_mapping.numel(), int(ignore_label), None, None, None, None,
                     orig_out.data_ptr() + 8 * r0, None, None, None, None, stream())

    res["x"] = [locs, torch.ones(M, 1, dtype=torch.float32, device=dev)]
    res["gather"] = gather
    res["offsets"] = _upload_i64(np.concatenate([[0], np.cumsum(counts)]).tolist(), dev)
    res["n_outside"] = n_outside
    res["aug_points_ls"] = list(src) if through else list(pts_out.split(counts))
    if has["seg_label"]:
        res["seg_label"] = seg_out
        res["orig_seg_label"] = list(seg_out.split(counts)) if through else list(orig_out.split(kcounts))
    if has["img_indices"]:
        res["img_indices"] = list(side["img_indices"]) if through else list(img_out.split(counts))
    for k in ps_keys:
        res[k] = ps_flat[k] if through else ps_out[k]
    if has["pseudo_label_3d"]:
        res["ori_pslabel_ls"] = list(ps_flat["pseudo_label_3d"].split(ns))
    # the reference's idxs: one flag per point that survives keep_in
    if through:
        idxs = list(torch.ones(total, dtype=torch.bool, device=dev).split(ns))
    elif has["keep_in"]:
        idxs = list(mask1.view(torch.bool).split(kcounts))
    else:
        idxs = [c["flags"][:sum(ns[c["s"]:c["e"]])].view(torch.bool) for c in chunks]
        idxs = [v for c, f in zip(chunks, idxs) for v in f.split(ns[c["s"]:c["e"]])]
    res["orig_points_idx"] = idxs
    if ema_input:
        res["ori_x"] = [ori_locs, torch.ones(Mo, 1, dtype=torch.float32, device=dev)]
        res["ori_keep_idx"] = list(side["keep_in"]) if has["keep_in"] else list(torch.ones(total, dtype=torch.bool, device=dev).split(ns))
        res["ori_idxs"] = idxs
    return res


def _refine_into(probs, labels, views, ignore_label, num_classes, dev):
    """One segmented call for at most 2 x MAXB (array, scan) pairs whose results go to the given int64 views."""
    c = 32 if num_classes is None else int(num_classes)
    S = len(labels)
    ws = workspace.get(query("mopa_refine_pseudo_labels_segmented_workspace_bytes", S, c), dev)
    pt, lt, ot = (host_ptrs(probs) if probs is not None else None), host_ptrs(labels), host_ptrs(views)
    nt = host_i32([t.numel() for t in labels])
    call("mopa_refine_pseudo_labels_segmented", host_addr(pt), host_addr(lt), _LABEL_DTYPES[labels[0].dtype], host_addr(nt), host_addr(ot),
         S, c, int(ignore_label), ptr(ws), ws.numel(), stream())
