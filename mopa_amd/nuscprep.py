"""nuScenes' offline preprocessing of a sweep on the device: the raw sweeps of a call (the ``.pcd.bin`` contents as loaded, the nine
calibration entries of the sample, the 3D boxes visible in the camera, optionally PatchWork++'s ground index list or a ground mask)
-> what ``preprocess`` (``mopa/data/nuscenes/preprocess.py:77-148`` with ``map_pointcloud_to_image``, ``projection.py:9-90``)
leaves in the pickle and ``nuscenes_dataloader.py:305-316`` makes of the ground list: the lidar points that fall into the front
camera's image, their image coordinates ``[row, col]``, the detection labels painted from the boxes, the keep mask over the raw
sweep, the composite ``proj_matrix`` and the ground mask of the kept points.  The outputs are the inputs of
``imageprep.prepare_batch`` (``points_img``) and ``scanprep.prepare_batch_3d`` (``points``, ``seg_labels``).

``prepare_scans_nuscenes`` runs this for the B samples with a fixed number of launches (``csrc/nuscprep.hip``: every kernel covers
all scans) and exactly ONE blocking read-back, of the B counts that size the outputs.  There is no CPU fallback.  Reading the
NuScenes database, the token filter of the boxes and ``category_to_detection_name`` are host string work and stay with the caller.

Arithmetic (fixture G15): float64 until the reference's cast; every matrix product is per element the fused
chain ``fma(a[K-1], b[K-1], ... fma(a1, b1, a0 * b0))``, which is what numpy's float64 ``@`` / ``np.dot`` computed on the host the
fixture was generated on.  The projection flow is pinned by running the reference's own function; the quaternion matrix,
``view_points``, ``Box.corners`` and ``points_in_box`` are written from the published definitions of pyquaternion and
nuscenes-devkit, which were not at hand: UNVERIFIED against the libraries themselves.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from ._lib import call, chunk_ranges, host_addr, host_i32, host_ptrs, ptr, query, stream
from ._prep import check_devices, ground_mask, image_size_wh, out_rows, read_counts, tensor_checker

_NAME = "prepare_scans_nuscenes"
CALIB_KEYS = ("lidar2ego_rotation", "ego2global_rotation_lidar", "ego2global_rotation_cam", "cam2ego_rotation",
              "lidar2ego_translation", "ego2global_translation_lidar", "ego2global_translation_cam", "cam2ego_translation",
              "cam_intrinsic")
_SHAPES = ((4,),) * 4 + ((3,),) * 4 + ((3, 3),)
NO_BOX = 10                    # seg_labels of a point in no labelled box: len(class_names_to_id) of preprocess.py:21-23


# ------------------------------------------------------------------------------------------------ host helpers (numpy only)
def rotation_matrix(q) -> np.ndarray:
    """pyquaternion's ``Quaternion(q).rotation_matrix`` from its published form: q = [w, x, y, z]; normalised unless
    ``abs(1 - q.q) < 1e-14``; ``(Q @ Qbar^T)[1:, 1:]``."""
    q = np.array(q, dtype=np.float64)
    ss = float(np.dot(q, q))
    if not abs(1.0 - ss) < 1e-14:
        n = np.sqrt(ss)
        if n > 0:
            q = q / n
    w, x, y, z = q
    Q = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    Qb = np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])
    return np.dot(Q, Qb.transpose())[1:, 1:]


def proj_matrix(calib) -> np.ndarray:
    """The composite (4, 4) float64 ``proj_mtx`` of ``projection.py:25-56``: intrinsics @ ego2cam^-1 @ global2ego^-1 @ ego2global @
    lidar2ego.  Host data in the reference too; numpy's own products (not pinned to a chain: compare with a tolerance)."""
    def rigid(rot, tr):
        m = np.eye(4)
        m[:3, :3] = rotation_matrix(calib[rot])
        m[:3, 3] = np.array(calib[tr], dtype=np.float64)
        return m

    lidar2ego = rigid("lidar2ego_rotation", "lidar2ego_translation")
    ego2global = rigid("ego2global_rotation_lidar", "ego2global_translation_lidar")
    global2ego = np.linalg.inv(rigid("ego2global_rotation_cam", "ego2global_translation_cam"))
    ego2cam = np.linalg.inv(rigid("cam2ego_rotation", "cam2ego_translation"))
    intr = np.eye(4)
    intr[:3, :3] = np.array(calib["cam_intrinsic"], dtype=np.float64)
    return intr @ (ego2cam @ global2ego @ ego2global @ lidar2ego)


# ------------------------------------------------------------------------------------------------ argument checks
def _check(samples, image_size, with_ground):
    """Types, dtypes and shapes first (so that a malformed call is named as such on any device), then the device.
    -> (W, H, ground form: None / "g_indices" / "g_mask", per sample (calib (37,), boxes (M, 11)))."""
    if not samples:
        raise ValueError(f"{_NAME}: no samples")
    w, h = image_size_wh(_NAME, image_size)
    for s in samples:
        if not isinstance(s, dict):
            raise TypeError(f"{_NAME}: every sample must be a dict, got {type(s).__name__}")
    for key in ("g_indices", "g_mask"):
        have = [s.get(key) is not None for s in samples]
        if any(have) and not all(have):
            raise ValueError(f"{_NAME}: either every sample of a call has `{key}` or none")
    first = samples[0]
    if first.get("g_indices") is not None and first.get("g_mask") is not None:
        raise ValueError(f"{_NAME}: `g_indices` and `g_mask` are two forms of one input; give one")
    form = "g_indices" if first.get("g_indices") is not None else "g_mask" if first.get("g_mask") is not None else None
    if with_ground and form is None:
        raise ValueError(f"{_NAME}: with_ground needs `g_indices` or `g_mask` in every sample")
    if with_ground is not None and not with_ground:
        form = None
    host = []
    tensor, tensors = tensor_checker(_NAME)

    def array(b, what, v, shape):
        if isinstance(v, torch.Tensor):
            raise TypeError(f"{_NAME}: {what} of sample {b} must be a host list or numpy array, got a torch tensor")
        try:
            a = np.array(v, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError(f"{_NAME}: {what} of sample {b} must be numbers of shape {shape}, got {type(v).__name__}") from None
        if a.shape != shape:
            raise ValueError(f"{_NAME}: {what} of sample {b} must have shape {shape}, got {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"{_NAME}: {what} of sample {b} is not finite")
        return a

    for b, s in enumerate(samples):
        scan = tensor(b, s, "scan", (torch.float32,), "float32")
        if scan.dim() != 2 or scan.shape[1] < 3:
            raise ValueError(f"{_NAME}: scan of sample {b} must be (N, 5) or (N, >= 3), got {tuple(scan.shape)}")
        n = scan.shape[0]
        calib = s.get("calib")
        if not isinstance(calib, dict):
            raise TypeError(f"{_NAME}: calib of sample {b} must be a dict of host lists or arrays, got {type(calib).__name__}")
        parts = []
        for key, shape in zip(CALIB_KEYS, _SHAPES):
            if key not in calib:
                raise ValueError(f"{_NAME}: calib of sample {b} lacks `{key}`")
            parts.append(array(b, f"calib[{key!r}]", calib[key], shape))
            if shape == (4,) and not np.any(parts[-1]):
                raise ValueError(f"{_NAME}: calib[{key!r}] of sample {b} is the zero quaternion")
        boxes = s.get("boxes")
        if boxes is None or isinstance(boxes, torch.Tensor):
            raise TypeError(f"{_NAME}: boxes of sample {b} must be a host (M, 10) float array, got {type(boxes).__name__}")
        boxes = np.asarray(boxes)
        if boxes.size == 0:
            boxes = np.zeros((0, 10))
        if boxes.ndim != 2 or boxes.shape[1] != 10 or boxes.dtype.kind not in "fiu":
            raise ValueError(f"{_NAME}: boxes of sample {b} must be (M, 10) [center, wlh, quaternion wxyz], got {boxes.shape} {boxes.dtype}")
        boxes = boxes.astype(np.float64)
        if not np.isfinite(boxes).all():
            raise ValueError(f"{_NAME}: boxes of sample {b} are not finite")
        if len(boxes) and not np.any(boxes[:, 6:], axis=1).all():
            raise ValueError(f"{_NAME}: boxes of sample {b} hold a zero quaternion")
        cls = s.get("box_class")
        if cls is None or isinstance(cls, torch.Tensor):
            raise TypeError(f"{_NAME}: box_class of sample {b} must be a host (M,) int array, got {type(cls).__name__}")
        cls = np.asarray(cls)
        if cls.size == 0:
            cls = np.zeros(0, np.int64)
        if cls.dtype.kind not in "iu":
            raise TypeError(f"{_NAME}: box_class of sample {b} must be integers, got {cls.dtype}")
        if cls.shape != (len(boxes),):
            raise ValueError(f"{_NAME}: box_class of sample {b} must be ({len(boxes)},) for {len(boxes)} boxes, got {cls.shape}")
        if len(cls) and (cls.min() < -1 or cls.max() > 255):
            raise ValueError(f"{_NAME}: box_class of sample {b} must lie in -1 (no detection class) .. 255")
        host.append((np.concatenate([p.reshape(-1) for p in parts]), np.concatenate([boxes, cls.astype(np.float64)[:, None]], 1)))
        if form == "g_indices":
            g = tensor(b, s, "g_indices", (torch.int32,), "int32")
            if g.dim() != 1:
                raise ValueError(f"{_NAME}: g_indices of sample {b} must be (G,), got {tuple(g.shape)}")
        if form == "g_mask":
            g = tensor(b, s, "g_mask", (torch.bool,), "bool")
            if tuple(g.shape) != (n,):
                raise ValueError(f"{_NAME}: g_mask of sample {b} must be ({n},) for {n} points, got {tuple(g.shape)}")
    check_devices(_NAME, tensors)
    return w, h, form, host


# ------------------------------------------------------------------------------------------------ the batch
def prepare_scans_nuscenes(samples, image_size=(1600, 900), with_ground=None) -> dict:
    """``preprocess`` (``preprocess.py:77-148``) for the B sweeps of one call, every stage as one launch for all of them.

    ``samples``: B dicts.  ``scan`` (N, 5) or (N, >= 3) float32 device tensor (the ``.pcd.bin`` as loaded; x, y, z are used);
    ``calib``: the nine entries of ``preprocess.py:93-103`` as host lists or arrays (quaternions wxyz); ``boxes``: host (M, 10)
    float64 ``[center, wlh, quaternion wxyz]`` in the lidar frame, already filtered to the boxes visible in the camera, in file
    order; ``box_class``: host (M,) int, the detection class id of each box, -1 for none (such a box labels nothing); optionally,
    for all samples or none, ``g_indices`` (G,) int32 device tensor (PatchWork++'s index list into the raw sweep, numpy's
    indexing) or ``g_mask`` (N,) bool device tensor (the form ``ground.estimate_ground_batch`` returns).  ``image_size`` = (W, H).
    ``with_ground``: None = return the ground mask when the samples carry one of the two; True = require it; False = leave it.

    Returns lists of B device tensors: ``points`` (Nk, 3) float32 (the raw lidar xyz), ``points_img`` (Nk, 2) float32
    ``[row, col]``, ``seg_labels`` (Nk,) uint8 (10 = in no labelled box), ``valid_mask`` (N,) bool, ``g_indices`` (Nk,) bool with
    ground; ``proj_matrix``: B host (4, 4) float64 arrays; and ``counts``, a (B,) int64 numpy array of Nk on the host.

    One blocking read-back per call (the counts).  A ground index outside its scan is refused after it (IndexError, as numpy)."""
    samples = list(samples)
    w, h, form, host = _check(samples, image_size, with_ground)
    B = len(samples)
    dev = samples[0]["scan"].device
    scans = [s["scan"].contiguous() for s in samples]
    ns = [t.shape[0] for t in scans]
    cols = [t.shape[1] for t in scans]
    rows = query("mopa_nuscprep_rows_per_block")
    N = sum(ns)
    flags = torch.empty(max(N, 1), dtype=torch.uint8, device=dev)           # the valid masks of all scans, one after the other

    chunks = []
    r0 = 0
    for s, e in chunk_ranges(B, query("mopa_nuscprep_max_scans")):
        Bc = e - s
        total = sum(ns[s:e])
        ms = [len(host[b][1]) for b in range(s, e)]
        M = sum(ms)
        c = {"s": s, "e": e, "B": Bc, "scan": host_ptrs(scans[s:e]), "n": host_i32(ns[s:e]), "cols": host_i32(cols[s:e]),
             "boxoff": host_i32(np.concatenate([[0], np.cumsum(ms)])), "gmask": None, "bad": None, "r0": r0}
        blob = np.concatenate([host[b][0] for b in range(s, e)] + [host[b][1].reshape(-1) for b in range(s, e)])
        c["in"] = torch.from_numpy(blob).to(dev)                             # the one upload: (Bc, 37) calibration | (M, 11) boxes
        c["table"] = torch.empty(max(query("mopa_nuscprep_table_bytes", Bc, M) // 8, 1), dtype=torch.float64, device=dev)
        nblk = sum(-(-n // rows) for n in ns[s:e])
        c["ws"] = torch.empty(query("mopa_nuscprep_workspace_bytes", nblk), dtype=torch.uint8, device=dev)
        c["counts"] = torch.empty(Bc + 1, dtype=torch.int64, device=dev)
        call("mopa_nuscprep_setup", ptr(c["in"]), ptr(c["in"], 37 * Bc) if M else None, Bc, M, ptr(c["table"]), stream())
        if form == "g_indices":
            c["gmask"], c["bad"] = ground_mask(call, [samples[b]["g_indices"] for b in range(s, e)], c["n"])
        elif form == "g_mask":
            c["gmask"] = torch.cat([samples[b]["g_mask"].reshape(-1) for b in range(s, e)] + [torch.zeros(1, dtype=torch.bool, device=dev)]).view(torch.uint8)
        call("mopa_nuscprep_count", host_addr(c["scan"]), host_addr(c["n"]), host_addr(c["cols"]), Bc, ptr(c["table"]), w, h,
             ptr(flags, r0), ptr(c["bad"]), ptr(c["counts"]), ptr(c["ws"]), c["ws"].numel(), stream())
        chunks.append(c)
        r0 += total

    # the one read-back: per chunk Nk of every scan, then the number of ground indices outside their scan
    counts = read_counts(_NAME, chunks, 1).reshape(-1)
    nk = [int(v) for v in counts]
    K = sum(nk)

    _rows = functools.partial(out_rows, K, device=dev)
    out = {"points": _rows(3), "img": _rows(2), "seg": _rows(dtype=torch.uint8), "g": _rows(dtype=torch.uint8) if form else (None, 0, None)}
    k0 = 0
    for c in chunks:
        at = {k: None if addr is None else addr + k0 * step for k, (_, step, addr) in out.items()}
        call("mopa_nuscprep_scatter", host_addr(c["scan"]), host_addr(c["n"]), host_addr(c["cols"]), host_addr(c["boxoff"]), c["B"],
             ptr(c["table"]), w, h, ptr(flags, c["r0"]), ptr(c["gmask"]), at["points"], at["img"], at["seg"], at["g"], ptr(c["ws"]),
             c["ws"].numel(), stream())
        k0 += sum(nk[c["s"]:c["e"]])

    res = {"points": list(out["points"][0].split(nk)), "points_img": list(out["img"][0].split(nk)), "seg_labels": list(out["seg"][0].split(nk)),
           "valid_mask": list(flags[:N].view(torch.bool).split(ns)), "proj_matrix": [proj_matrix(s["calib"]) for s in samples], "counts": counts}
    if form:
        res["g_indices"] = list(out["g"][0].view(torch.bool).split(nk))
    return res
