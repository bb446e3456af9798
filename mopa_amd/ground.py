"""Ground estimation on the device: the per-point ground mask that Valid Ground-based Insertion (``mopa_amd/vgi.py``) takes as
``g_indices``, computed from the raw scans of an iteration instead of being loaded from an offline pass.

The reference obtains this mask from Patchwork++, a third-party C++ module: offline for every shipped config
(``g_indices_dir``, written by ``mopa/data/*/preprocess.py``), or on the host inside ``obj_on_road`` when no mask is given
(``mopa/data/mixmatch_ss.py:380-388``).  What runs here is NOT Patchwork++ and does not reproduce its bits.  It is the published
Patchwork core as DESIGN.md section 4 states it: a concentric zone model of 504 patches, per patch a plane fitted from the lowest
points (LPR, seed set, three rounds of fit + classify) and three tests on the final fit (uprightness, elevation, flatness), all in
float64.  Not included: adaptive thresholds across frames, reflected-noise removal beyond the zone-0 cut, vertical-plane fitting,
the temporal revert.  The yardstick is the numpy restatement ``tests/_ground_reference.py``.

``estimate_ground_batch`` runs all scans of a list with one library call (``csrc/ground.hip``: every kernel covers all scans; the
number of launches does not depend on the batch size), reads nothing back, and has no CPU fallback.  The estimate is opt-in:
``vgi.point_mixmatch`` still raises without a mask; pass ``g_indices=estimate_ground(pc)``.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from ._lib import call, ptr, query, stream

_NAME = "estimate_ground"


@dataclasses.dataclass(frozen=True)
class GroundParams:
    """``sensor_height`` in metres above the ground (1.84 nuScenes, 1.73 SemanticKITTI); the rest are the defaults of DESIGN.md
    section 4.  The zone model itself (4 zones of 2, 4, 4, 4 rings and 16, 32, 54, 32 sectors: 504 patches) is fixed."""
    sensor_height: float
    rmin: float = 2.7
    rmax: float = 80.0
    num_min_pts: int = 10
    num_lpr: int = 20
    num_iter: int = 3
    th_seeds: float = 0.125
    th_dist: float = 0.125
    uprightness: float = 0.707
    elevation: tuple = (0.523, 0.746, 0.879, 1.125)
    flatness: tuple = (0.0005, 0.000725, 0.001, 0.001)
    noise_cut: float = 1.1                      # zone-0 points below -noise_cut * sensor_height are reflections: in no patch

    def __post_init__(self):
        for k in ("sensor_height", "rmin", "rmax", "th_seeds", "th_dist", "uprightness", "noise_cut"):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                raise ValueError(f"GroundParams: {k} must be a finite number, got {v!r}")
        if not 0 < self.rmin < self.rmax:
            raise ValueError(f"GroundParams: need 0 < rmin < rmax, got {self.rmin!r}, {self.rmax!r}")
        for k, lo in (("num_min_pts", 3), ("num_lpr", 1), ("num_iter", 1)):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or v > (64 if k == "num_iter" else 1 << 20):
                raise ValueError(f"GroundParams: {k} must be an integer >= {lo}, got {v!r}")
        for k in ("elevation", "flatness"):
            v = getattr(self, k)
            if len(v) != 4 or not all(np.isfinite(float(x)) for x in v):
                raise ValueError(f"GroundParams: {k} must hold four finite numbers (global rings 0..3), got {v!r}")

    def as_array(self) -> np.ndarray:
        """The float64 record ``mopa_ground_estimate`` takes."""
        return np.array([self.sensor_height, self.rmin, self.rmax, self.th_seeds, self.th_dist, self.uprightness, self.noise_cut,
                         *self.elevation, *self.flatness, self.num_min_pts, self.num_lpr, self.num_iter], np.float64)


# ------------------------------------------------------------------------------------------------ argument checks
def _check(point_sets, counts, params):
    """Types, dtypes and shapes first (so that a malformed call is named as such on any machine), then the device.
    -> (list of arrays / tensors, counts or None)"""
    if not isinstance(params, GroundParams):
        raise TypeError(f"{_NAME}: params must be a GroundParams, got {type(params).__name__}")
    if counts is not None:
        sets = [point_sets]
        try:
            counts = [int(c) for c in counts]
        except (TypeError, ValueError):
            raise TypeError(f"{_NAME}: counts must be a sequence of integers, got {counts!r}") from None
        if any(c < 0 for c in counts):
            raise ValueError(f"{_NAME}: counts must not be negative, got {counts}")
    else:
        if isinstance(point_sets, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{_NAME}: point_sets must be a list of (N, >=3) arrays (or one concatenated array with `counts`)")
        sets = list(point_sets)
    if not sets:
        raise ValueError(f"{_NAME}: no scans")
    for b, t in enumerate(sets):
        if not isinstance(t, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{_NAME}: scan {b} must be a numpy array or a torch tensor, got {type(t).__name__}")
        dtype = t.dtype
        if dtype in (torch.float16, torch.bfloat16, np.dtype(np.float16)):
            raise TypeError(f"{_NAME}: scan {b} is {dtype}: half precision is refused (coordinates up to 80 m need float32)")
        if dtype not in (torch.float32, np.dtype(np.float32)):
            raise TypeError(f"{_NAME}: scan {b} must be float32, got {dtype}")
        if t.ndim != 2 or t.shape[1] < 3:
            raise ValueError(f"{_NAME}: scan {b} must be (N, >=3), got {tuple(t.shape)}")
        if t.shape[1] != sets[0].shape[1]:
            raise ValueError(f"{_NAME}: scan {b} has {t.shape[1]} columns, scan 0 has {sets[0].shape[1]}; one width per call")
    if counts is not None and sum(counts) != sets[0].shape[0]:
        raise ValueError(f"{_NAME}: counts add up to {sum(counts)}, the concatenated points have {sets[0].shape[0]} rows")
    if sum(t.shape[0] for t in sets) >= 1 << 30:
        raise ValueError(f"{_NAME}: at most 2^30 - 1 points per call")
    if len(counts if counts is not None else sets) > 65535:
        raise ValueError(f"{_NAME}: at most 65535 scans per call")
    devs = {t.device for t in sets if isinstance(t, torch.Tensor) and t.is_cuda}
    if len(devs) > 1:
        raise ValueError(f"{_NAME}: the scans are on {sorted(map(str, devs))}; all tensors of a call must be on one device")
    return sets, counts


# ------------------------------------------------------------------------------------------------ the batch
def estimate_ground_batch(point_sets, params: GroundParams, counts=None, device=None) -> list:
    """The ground masks of the B scans of an iteration: a list of B uint8 device tensors ``(N_b,)``, 1 = ground.

    ``point_sets``: B arrays ``(N_b, >=3)`` float32 (x, y, z in the sensor frame, z up; further columns are ignored), numpy arrays
    on the host or torch tensors on the host or the device -- or, with ``counts``, ONE such array holding the scans behind each
    other and the B row counts (``kittiprep.prepare_scans_kitti``'s ``torch.cat(points)`` and ``counts[:, 1]``).  Host inputs are
    uploaded once, as one array.  One library call for the whole list, nothing is read back; the masks are views of one buffer."""
    sets, counts = _check(point_sets, counts, params)
    dev = next((t.device for t in sets if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError(f"{_NAME}: the estimate runs on the GPU (there is no CPU fallback), got device {dev}")
    ns = counts if counts is not None else [t.shape[0] for t in sets]
    if all(isinstance(t, np.ndarray) for t in sets):
        host = sets[0] if len(sets) == 1 else np.concatenate(sets, 0)
        pts = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
    else:
        parts = [(torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).to(dev) for t in sets]
        pts = (parts[0] if len(parts) == 1 else torch.cat(parts, 0)).contiguous()
    total, cols, B = pts.shape[0], pts.shape[1], len(ns)
    mask = torch.empty(total, dtype=torch.uint8, device=dev)
    if total > 0:
        rows = query("mopa_ground_rows_per_block")
        row0 = np.concatenate([[0], np.cumsum(ns)])
        blk0 = np.concatenate([[0], np.cumsum([-(-n // rows) for n in ns])])
        nblk = int(blk0[-1])
        tab = torch.from_numpy(np.concatenate([row0, blk0]).astype(np.int32)).to(dev)
        ws = torch.empty(query("mopa_ground_workspace_bytes", total, nblk), dtype=torch.uint8, device=dev)
        prm = params.as_array()
        assert prm.size == query("mopa_ground_num_params")
        with torch.cuda.device(dev):
            call("mopa_ground_estimate", ptr(pts), cols, ptr(tab), B, total, nblk, prm.ctypes.data, ptr(mask), ptr(ws), ws.numel(), stream())
    return list(mask.split(list(ns)))


def estimate_ground(points, params: GroundParams, device=None) -> torch.Tensor:
    """The ground mask of one scan ``(N, >=3)`` float32, host or device: a uint8 device tensor ``(N,)``, 1 = ground.  What
    ``vgi.point_mixmatch(..., g_indices=...)`` and ``kittiprep``'s ground input take, as it is."""
    if not isinstance(points, (torch.Tensor, np.ndarray)):
        raise TypeError(f"{_NAME}: points must be a numpy array or a torch tensor, got {type(points).__name__}")
    return estimate_ground_batch([points], params, device=device)[0]


# ------------------------------------------------------------------------------------------------ the offline form
def ground_indices(mask) -> torch.Tensor:
    """The ascending int32 indices of the ground points: the content of one of the reference's ``g_indices`` ``.bin`` files."""
    m = torch.as_tensor(mask)
    if m.dim() != 1 or m.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"ground_indices: the mask must be a (N,) uint8 or bool array, got {tuple(m.shape)} {m.dtype}")
    return torch.nonzero(m).squeeze(1).to(torch.int32)


def dump_g_indices(path, mask) -> int:
    """Write the mask as the reference's datasets read it back: ``np.fromfile(path, dtype=np.int32)`` gives the ground points'
    indices into the raw scan.  -> the number of indices written."""
    idx = ground_indices(mask).cpu().numpy().astype(np.int32)
    idx.tofile(path)
    return int(idx.size)
