"""The object bank of Valid Ground-based Insertion (``mopa_amd/vgi.py``: ``obj_pc_ls`` / ``obj_label_ls``), built on the device from
labelled scans -- the source scans of the very iteration that inserts them, or a whole labelled set as the reference's offline pass.

The reference makes the bank offline (``mopa/data/waymo/obj_point_extract.py``): per scan and class it runs
``sklearn.cluster.DBSCAN(eps=4, min_samples=5).fit_predict`` on the class's points, walks ``np.unique`` of the labels (the noise
label -1 included: the noise points of a segment form one "instance"), keeps those whose mean range is at most ``max_distance``
until every class holds ``max_num``, and writes them as ``<class_name>/NNNNN.bin``; the datasets' ``obj_sampling`` draws from the
files.  ``extract_instances_batch`` computes the same labels, exactly (``csrc/objects.hip``; yardstick
``tests/_objects_reference.py``), for all scans and classes of a call with one library call and one read-back of three counters;
``ObjectBank`` holds the cap, the file layout and the draw.  The one stated deviation: rows with a non-finite coordinate (or one
beyond ``2^20 eps``), on which sklearn raises, are in no instance and are counted in ``n_rejected``.  There is no CPU fallback.
"""
from __future__ import annotations

import dataclasses
import glob
import os

import numpy as np
import torch

from ._lib import call, ptr, query, stream

_NAME = "extract_instances"
_LABEL_DTYPES = {torch.int64: 8, torch.int32: 4, torch.uint8: 1, np.dtype(np.int64): 8, np.dtype(np.int32): 4, np.dtype(np.uint8): 1}
MAX_CLASSES = 32


@dataclasses.dataclass(frozen=True)
class ClusterParams:
    """The reference's values: ``DBSCAN(eps=4, min_samples=5)``, ``max_distance = 15``.  ``include_noise``: the noise points of a
    (scan, class) are one instance (id -1), as the reference's ``np.unique`` loop has it; False drops that group."""
    eps: float = 4.0
    min_samples: int = 5
    max_distance: float = 15.0
    include_noise: bool = True

    def __post_init__(self):
        for k in ("eps", "max_distance"):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                raise ValueError(f"ClusterParams: {k} must be a finite number, got {v!r}")
        if not self.eps > 0:
            raise ValueError(f"ClusterParams: eps must be positive, got {self.eps!r}")
        v = self.min_samples
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or v > 1 << 20:
            raise ValueError(f"ClusterParams: min_samples must be an integer >= 1, got {v!r}")
        if not isinstance(self.include_noise, (bool, np.bool_)):
            raise ValueError(f"ClusterParams: include_noise must be a bool, got {self.include_noise!r}")

    def as_array(self) -> np.ndarray:
        """The float64 record ``mopa_objects_extract`` takes."""
        return np.array([self.eps, self.min_samples, self.max_distance, 1.0 if self.include_noise else 0.0], np.float64)


@dataclasses.dataclass
class Instances:
    """What ``extract_instances_batch`` returns; every array is a device tensor.  ``labels``: per scan int32 ``(N_b,)``, -2 = no
    requested class or rejected, -1 = noise, >= 0 = the cluster id inside its (scan, class).  ``table`` int32 ``(M, 4)``: scan,
    class position in ``class_ids``, instance id (-1 = the noise group), points -- ordered by scan, class position, id.
    ``offsets`` int32 ``(M + 1,)``: the points of instance i are ``points[offsets[i]:offsets[i + 1]]``, in the scan's row order.
    ``mean_range`` float64 ``(M,)``, ``keep`` uint8 ``(M,)`` = mean_range <= max_distance.  ``n_rejected``: rows of a requested
    class left out for a non-finite or out-of-grid coordinate."""
    labels: list
    table: torch.Tensor
    offsets: torch.Tensor
    mean_range: torch.Tensor
    keep: torch.Tensor
    points: torch.Tensor
    n_rejected: int
    class_ids: tuple

    def __len__(self):
        return self.table.shape[0]


# ------------------------------------------------------------------------------------------------ argument checks
def _check_class_ids(class_ids):
    try:
        ids = [c for c in class_ids]
    except TypeError:
        raise TypeError(f"{_NAME}: class_ids must be a sequence of integers, got {class_ids!r}") from None
    if any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) for c in ids):
        raise TypeError(f"{_NAME}: class_ids must be integers, got {ids!r}")
    ids = [int(c) for c in ids]
    if not ids:
        raise ValueError(f"{_NAME}: no class ids")
    if len(ids) > MAX_CLASSES:
        raise ValueError(f"{_NAME}: at most {MAX_CLASSES} classes per call, got {len(ids)}")
    if len(set(ids)) != len(ids):
        raise ValueError(f"{_NAME}: class_ids must be distinct, got {ids}")
    if any(c < -(1 << 31) or c >= 1 << 31 for c in ids):
        raise ValueError(f"{_NAME}: class ids must fit 32 bits, got {ids}")
    return ids


def _check(point_sets, label_sets, class_ids, params, counts):
    """Types, dtypes and shapes first (so that a malformed call is named as such on any machine), then the device.
    -> (point arrays, label arrays, class ids, counts or None)"""
    if not isinstance(params, ClusterParams):
        raise TypeError(f"{_NAME}: params must be a ClusterParams, got {type(params).__name__}")
    ids = _check_class_ids(class_ids)
    if counts is not None:
        sets, labs = [point_sets], [label_sets]
        try:
            counts = [int(c) for c in counts]
        except (TypeError, ValueError):
            raise TypeError(f"{_NAME}: counts must be a sequence of integers, got {counts!r}") from None
        if any(c < 0 for c in counts):
            raise ValueError(f"{_NAME}: counts must not be negative, got {counts}")
    else:
        if isinstance(point_sets, (torch.Tensor, np.ndarray)) or isinstance(label_sets, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{_NAME}: point_sets and label_sets must be lists of arrays (or one concatenated array each with `counts`)")
        sets, labs = list(point_sets), list(label_sets)
    if not sets:
        raise ValueError(f"{_NAME}: no scans")
    if len(labs) != len(sets):
        raise ValueError(f"{_NAME}: {len(sets)} scans but {len(labs)} label arrays")
    for b, (t, l) in enumerate(zip(sets, labs)):
        if not isinstance(t, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{_NAME}: scan {b} must be a numpy array or a torch tensor, got {type(t).__name__}")
        if not isinstance(l, (torch.Tensor, np.ndarray)):
            raise TypeError(f"{_NAME}: the labels of scan {b} must be a numpy array or a torch tensor, got {type(l).__name__}")
        if t.dtype in (torch.float16, torch.bfloat16, np.dtype(np.float16)):
            raise TypeError(f"{_NAME}: scan {b} is {t.dtype}: half precision is refused (the distances are taken from float32 coordinates)")
        if t.dtype not in (torch.float32, np.dtype(np.float32)):
            raise TypeError(f"{_NAME}: scan {b} must be float32, got {t.dtype}")
        if t.ndim != 2 or t.shape[1] < 3:
            raise ValueError(f"{_NAME}: scan {b} must be (N, >=3), got {tuple(t.shape)}")
        if t.shape[1] != sets[0].shape[1]:
            raise ValueError(f"{_NAME}: scan {b} has {t.shape[1]} columns, scan 0 has {sets[0].shape[1]}; one width per call")
        if l.dtype not in _LABEL_DTYPES:
            raise TypeError(f"{_NAME}: the labels of scan {b} must be int64, int32 or uint8, got {l.dtype}")
        if _LABEL_DTYPES[l.dtype] != _LABEL_DTYPES[labs[0].dtype]:
            raise TypeError(f"{_NAME}: the labels of scan {b} are {l.dtype}, those of scan 0 {labs[0].dtype}; one dtype per call")
        if l.ndim != 1 or l.shape[0] != t.shape[0]:
            raise ValueError(f"{_NAME}: the labels of scan {b} must be ({t.shape[0]},), got {tuple(l.shape)}")
    if counts is not None and sum(counts) != sets[0].shape[0]:
        raise ValueError(f"{_NAME}: counts add up to {sum(counts)}, the concatenated points have {sets[0].shape[0]} rows")
    if sum(t.shape[0] for t in sets) >= 1 << 28:
        raise ValueError(f"{_NAME}: at most 2^28 - 1 points per call")
    if len(counts if counts is not None else sets) * len(ids) > 65535:
        raise ValueError(f"{_NAME}: scans x classes must not exceed 65535")
    devs = {t.device for t in sets + labs if isinstance(t, torch.Tensor) and t.is_cuda}
    if len(devs) > 1:
        raise ValueError(f"{_NAME}: the inputs are on {sorted(map(str, devs))}; all tensors of a call must be on one device")
    return sets, labs, ids, counts


def _cat(parts, dev):
    if all(isinstance(t, np.ndarray) for t in parts):
        host = parts[0] if len(parts) == 1 else np.concatenate(parts, 0)
        return torch.from_numpy(np.ascontiguousarray(host)).to(dev)
    ts = [(torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).to(dev) for t in parts]
    return (ts[0] if len(ts) == 1 else torch.cat(ts, 0)).contiguous()


# ------------------------------------------------------------------------------------------------ the batch
def extract_instances_batch(point_sets, label_sets, class_ids, params: ClusterParams, counts=None, device=None) -> Instances:
    """The DBSCAN instances of the classes ``class_ids`` in B labelled scans.

    ``point_sets``: B arrays ``(N_b, >=3)`` float32 (x, y, z first; every column is carried into ``points``), numpy arrays or torch
    tensors, host or device -- or, with ``counts``, ONE such array holding the scans behind each other and the B row counts.
    ``label_sets``: the per-point labels in the same form, int64, int32 or uint8.  ``class_ids``: at most 32 distinct integers,
    B x len(class_ids) <= 65535.  One library call for everything and one read-back (three counters, to size the views)."""
    sets, labs, ids, counts = _check(point_sets, label_sets, class_ids, params, counts)
    dev = next((t.device for t in sets + labs if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError(f"{_NAME}: the extraction runs on the GPU (there is no CPU fallback), got device {dev}")
    ns = counts if counts is not None else [t.shape[0] for t in sets]
    pts, lab = _cat(sets, dev), _cat(labs, dev)
    total, cols, B, C = pts.shape[0], pts.shape[1], len(ns), len(ids)
    out_labels = torch.empty(total, dtype=torch.int32, device=dev)
    if total == 0:
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)   # noqa: E731
        return Instances(list(out_labels.split(list(ns))), z(0, 4, dtype=torch.int32), z(1, dtype=torch.int32), z(0, dtype=torch.float64),
                         z(0, dtype=torch.uint8), z(0, cols, dtype=torch.float32), 0, tuple(ids))
    rows = query("mopa_objects_rows_per_block")
    row0 = np.concatenate([[0], np.cumsum(ns)])
    blk0 = np.concatenate([[0], np.cumsum([-(-n // rows) for n in ns])])
    nblk = int(blk0[-1])
    tab = torch.from_numpy(np.concatenate([row0, blk0]).astype(np.int32)).to(dev)
    cap = query("mopa_objects_max_instances", total, B, C)
    table = torch.empty(cap, 4, dtype=torch.int32, device=dev)
    offsets = torch.empty(cap + 1, dtype=torch.int32, device=dev)
    mean_range = torch.empty(cap, dtype=torch.float64, device=dev)
    keep = torch.empty(cap, dtype=torch.uint8, device=dev)
    points = torch.empty(total, cols, dtype=torch.float32, device=dev)
    counters = torch.empty(3, dtype=torch.int32, device=dev)
    ws = torch.empty(query("mopa_objects_workspace_bytes", total, nblk, B, C), dtype=torch.uint8, device=dev)
    prm = params.as_array()
    assert prm.size == query("mopa_objects_num_params")
    cls = np.asarray(ids, np.int32)
    with torch.cuda.device(dev):
        call("mopa_objects_extract", ptr(pts), cols, ptr(lab), _LABEL_DTYPES[lab.dtype], ptr(tab), B, total, nblk, cls.ctypes.data, C,
             prm.ctypes.data, ptr(out_labels), ptr(table), ptr(offsets), ptr(mean_range), ptr(keep), ptr(points), ptr(counters), ptr(ws),
             ws.numel(), stream())
    n_rejected, M, n_grouped = (int(v) for v in counters.cpu())          # the one read-back
    return Instances(list(out_labels.split(list(ns))), table[:M], offsets[:M + 1], mean_range[:M], keep[:M], points[:n_grouped],
                     n_rejected, tuple(ids))


def extract_instances(points, labels, class_ids, params: ClusterParams, device=None) -> Instances:
    """The one-scan form: ``points`` ``(N, >=3)`` float32 and ``labels`` ``(N,)``, host or device."""
    if not isinstance(points, (torch.Tensor, np.ndarray)):
        raise TypeError(f"{_NAME}: points must be a numpy array or a torch tensor, got {type(points).__name__}")
    if not isinstance(labels, (torch.Tensor, np.ndarray)):
        raise TypeError(f"{_NAME}: labels must be a numpy array or a torch tensor, got {type(labels).__name__}")
    return extract_instances_batch([points], [labels], class_ids, params, device=device)


# ------------------------------------------------------------------------------------------------ the bank
class ObjectBank:
    """The bank the reference keeps as a folder per class: ``class_names[i]`` holds instances of class ``class_ids[i]``, at most
    ``max_num`` each.  File reading and writing is host work; the instances come from ``extract_instances_batch``."""

    def __init__(self, class_names, class_ids, max_num: int):
        self.class_names = [str(n) for n in class_names]
        self.class_ids = _check_class_ids(class_ids)
        if len(self.class_names) != len(self.class_ids) or len(set(self.class_names)) != len(self.class_names):
            raise ValueError(f"ObjectBank: need one distinct name per class id, got {self.class_names} for {self.class_ids}")
        if isinstance(max_num, bool) or not isinstance(max_num, (int, np.integer)) or max_num < 1:
            raise ValueError(f"ObjectBank: max_num must be a positive integer, got {max_num!r}")
        self.max_num = int(max_num)
        self.objects = {n: [] for n in self.class_names}    # class name -> list of (n, cols) float32 host arrays

    def full(self) -> bool:
        return sum(len(v) for v in self.objects.values()) >= len(self.class_names) * self.max_num

    def add(self, instances: Instances) -> bool:
        """Take the kept instances in the reference's order -- scan, then class, then instance id (noise first) -- while their
        class holds fewer than ``max_num``; like the reference, stop after the (scan, class) that fills the bank.  -> full()."""
        if not isinstance(instances, Instances):
            raise TypeError(f"ObjectBank.add: expected Instances, got {type(instances).__name__}")
        if list(instances.class_ids) != self.class_ids:
            raise ValueError(f"ObjectBank.add: the instances are of classes {list(instances.class_ids)}, the bank of {self.class_ids}")
        if self.full():
            return True
        table = instances.table.cpu().numpy()
        offsets = instances.offsets.cpu().numpy()
        keep = instances.keep.cpu().numpy()
        points = instances.points.cpu().numpy()
        for i in range(table.shape[0]):
            if i > 0 and (table[i, 0], table[i, 1]) != (table[i - 1, 0], table[i - 1, 1]) and self.full():
                break                                       # the reference tests the total after every (scan, class)
            held = self.objects[self.class_names[table[i, 1]]]
            if keep[i] and len(held) < self.max_num:
                held.append(points[offsets[i]:offsets[i + 1]].copy())
        return self.full()

    def dump(self, save_dir) -> int:
        """``<save_dir>/<class_name>/NNNNN.bin``, numbered from 00001, float32 -- the reference's files.  -> files written."""
        n = 0
        for name in self.class_names:
            os.makedirs(os.path.join(save_dir, name), exist_ok=True)
            for k, o in enumerate(self.objects[name]):
                np.ascontiguousarray(o, np.float32).tofile(os.path.join(save_dir, name, "{:05d}.bin".format(k + 1)))
                n += 1
        return n

    @classmethod
    def load(cls, obj_root_dir, class_names, class_ids=None, cols: int = 4) -> "ObjectBank":
        """Read a bank as the datasets do: per class ``sorted(glob("*.bin"))``, float32 rows of ``cols`` values."""
        names = [str(n) for n in class_names]
        bank = cls(names, list(range(len(names))) if class_ids is None else class_ids, 1)
        for name in names:
            files = sorted(glob.glob(os.path.join(obj_root_dir, name, "*.bin")))
            bank.objects[name] = [np.fromfile(f, dtype=np.float32).reshape((-1, cols)) for f in files]
        bank.max_num = max(1, max(len(v) for v in bank.objects.values()))
        return bank

    def sample(self, obj_class, label_value):
        """``obj_sampling`` of the datasets: one ``np.random.choice(len(bank[obj_class]), 1)``, -> (obj_pc float32, obj_label
        float64 = ones * label_value)."""
        held = self.objects[obj_class]
        k = np.random.choice(len(held), 1)
        obj_pc = held[k[0]]
        if np.any(np.isnan(obj_pc)):
            raise AssertionError("Found Nan object points: {} {}".format(obj_class, int(k[0])))
        return obj_pc, np.ones(obj_pc.shape[0]) * label_value
