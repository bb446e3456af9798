"""Validation metrics on the device -- the reference's ``Evaluator`` (``mopa/data/utils/evaluate.py``) and the metric block of
``validate()`` (``mopa/data/utils/validate.py:112-131,140-170,184-185``) without their host round trips:

* ``Evaluator(class_names, labels=None)``: the reference's interface (``update``, ``batch_update``, ``confusion_matrix``,
  ``overall_acc``, ``overall_iou``, ``class_seg_acc``, ``class_iou``, ``print_table``, ``save_table``) over an int64 confusion
  matrix that stays on the device until a metric is read; ``all_reduce(group)`` sums it over ranks (exact).
* ``evaluate_batch(logit_2d, logit_3d, label, evaluators, pselab=False)``: one kernel pass over a batch's logits
  (csrc/evaluate.hip) -- 2D / 3D / xM (/ entropy-fused) confusion matrices, the two logged entropy means and CE losses as 0-d
  device tensors, optionally the pseudo-label dump.

Deviations from the reference: ``update`` does not write ``num_classes`` into the caller's label array
(the reference mutates ``gt_label`` in place, evaluate.py:22), and a scan none of whose ground-truth values is in ``labels``
adds nothing instead of raising sklearn's ValueError (checking would need a host sync).
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call, ptr, query, stream, workspace

MAXC = 64                                     # csrc/evaluate.hip EV_MAXC: classes of the logits and matrix size
KINDS = ("2D", "3D", "2D+3D", "2D+3D_ety")    # evaluate_batch's matrices, in the kernel's order
_MAX_LUT = 1 << 16


def _plain_table(header, rows, floatfmt):
    """A psql-style table without tabulate: text left-aligned, numbers right-aligned."""
    cells = [[("{:" + floatfmt + "}").format(v) if isinstance(v, float) else str(v) for v in r] for r in rows]
    num = [not isinstance(v, str) for v in (rows[0] if rows else [""] * len(header))]
    w = [max([len(h)] + [len(r[j]) for r in cells]) for j, h in enumerate(header)]
    line = "+" + "+".join("-" * (x + 2) for x in w) + "+"

    def fmt(r, align_num):
        return "| " + " | ".join(c.rjust(w[j]) if align_num and num[j] else c.ljust(w[j]) for j, c in enumerate(r)) + " |"
    out = [line, fmt(header, False), "|" + "+".join("-" * (x + 2) for x in w) + "|"]
    out += [fmt(r, True) for r in cells]
    out.append(line)
    return "\n".join(out)


class Evaluator:
    """Confusion-matrix evaluator with the reference's interface; the matrix is int64 on the device (exact counts)."""

    def __init__(self, class_names, labels=None):
        self.class_names = tuple(class_names)
        self.num_classes = len(self.class_names)
        if not 0 < self.num_classes <= MAXC:
            raise ValueError(f"Evaluator: {self.num_classes} classes; the device kernels take 1..{MAXC}")
        self.labels = np.arange(self.num_classes) if labels is None else np.array(labels)
        if self.labels.shape != (self.num_classes,):
            raise ValueError("Evaluator: labels must list one value per class name")
        self._lut_host = None                 # None = identity: class value c is matrix index c
        if labels is not None:
            lab = self.labels.astype(np.int64)
            if (lab < 0).any() or lab.max() >= _MAX_LUT:
                raise ValueError(f"Evaluator: labels must be class values in [0, {_MAX_LUT})")
            lut = np.full(int(lab.max()) + 1, -1, np.int32)
            for j, v in enumerate(lab):       # sklearn's {label: index}: a repeated label keeps its last index
                lut[v] = j
            self._lut_host = torch.from_numpy(lut)
        self._lut = {}                        # device -> int32 table
        self._conf = None                     # (L, L) int64, on the device of the first update

    # ------------------------------------------------------------------ device state
    def _lut_on(self, dev):
        if self._lut_host is None:
            return None
        t = self._lut.get(dev)
        if t is None:
            pinned = self._lut_host.pin_memory()       # asynchronous upload: no host sync even on the first call
            t = self._lut[dev] = pinned.to(dev, non_blocking=True)
            self._lut[("pinned", dev)] = pinned        # kept alive until long after the copy
        return t

    def _matrix(self, dev):
        if self._conf is None:
            self._conf = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=dev)
        elif self._conf.device != dev:
            raise ValueError(f"Evaluator: the matrix lives on {self._conf.device}, the inputs on {dev}")
        return self._conf

    def _device(self, *xs):
        for x in xs:
            if isinstance(x, torch.Tensor) and x.is_cuda:
                return x.device
        if self._conf is not None and self._conf.is_cuda:
            return self._conf.device
        return torch.device("cuda", torch.cuda.current_device())

    def same_table(self, other: "Evaluator") -> bool:
        return self.num_classes == other.num_classes and np.array_equal(self.labels, other.labels)

    # ------------------------------------------------------------------ reference interface
    def update(self, pred_label, gt_label):
        """Add one scan: rows = ground truth, columns = prediction; ground truth -100 and values outside ``labels`` are
        dropped.  numpy arrays are uploaded; device tensors are counted without a host sync."""
        dev = self._device(pred_label, gt_label)
        pred, gt = _i64(pred_label, dev), _i64(gt_label, dev)
        if pred.numel() != gt.numel():
            raise ValueError(f"Evaluator.update: {pred.numel()} predictions for {gt.numel()} labels")
        conf = self._matrix(dev)
        if pred.numel() == 0:
            return
        lut = self._lut_on(dev)
        call("mopa_confusion_update", ptr(pred), ptr(gt), pred.numel(), ptr(lut), 0 if lut is None else lut.numel(),
             self.num_classes, ptr(conf), stream())

    def batch_update(self, pred_labels, gt_labels):
        if len(pred_labels) != len(gt_labels):
            raise ValueError("Evaluator.batch_update: as many predictions as labels")
        for p, g in zip(pred_labels, gt_labels):
            self.update(p, g)

    def all_reduce(self, group=None):
        """Sum the matrix over the ranks of ``group`` (integer: exact), so each rank can evaluate its own shard."""
        import torch.distributed as dist
        if self._conf is None:
            on_gpu = dist.get_backend(group) == "nccl"
            self._matrix(torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu"))
        dist.all_reduce(self._conf, group=group)

    @property
    def confusion_matrix(self) -> np.ndarray:
        """(L, L) float64 on the host, like the reference's (the one host read of the accumulated counts)."""
        if self._conf is None:
            return np.zeros((self.num_classes, self.num_classes))
        return self._conf.cpu().numpy().astype(np.float64)

    @confusion_matrix.setter
    def confusion_matrix(self, value):
        v = np.asarray(value, dtype=np.float64)
        if v.shape != (self.num_classes, self.num_classes) or not np.array_equal(v, np.round(v)):
            raise ValueError("Evaluator.confusion_matrix: an (L, L) matrix of counts")
        dev = self._conf.device if self._conf is not None else torch.device("cpu")
        self._conf = torch.from_numpy(v.astype(np.int64)).to(dev)

    @property
    def overall_acc(self):
        cm = self.confusion_matrix
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.float64(np.trace(cm) / cm.sum())

    @property
    def overall_iou(self):
        """Mean over ALL classes with NaN IoU counted as 0 (evaluate.py:37-41)."""
        iou = np.array(self.class_iou, dtype=np.float64)
        iou[np.isnan(iou)] = 0
        return np.float64(iou.mean())

    @property
    def class_seg_acc(self):
        cm = self.confusion_matrix
        with np.errstate(divide="ignore", invalid="ignore"):
            return list(np.diag(cm) / cm.sum(1))          # 0 / 0 -> NaN

    @property
    def class_iou(self):
        cm = self.confusion_matrix
        tp = np.diag(cm)
        union = cm.sum(0) + cm.sum(1) - tp
        with np.errstate(divide="ignore", invalid="ignore"):
            return list(np.where(union == 0, np.nan, tp / union))

    def print_table(self):
        header = ["Class", "Accuracy", "IOU", "Total"]
        cm = self.confusion_matrix
        acc, iou = self.class_seg_acc, self.class_iou
        rows = [[name, float(acc[i] * 100), float(iou[i] * 100), int(cm[i].sum())] for i, name in enumerate(self.class_names)]
        try:
            from tabulate import tabulate
        except ImportError:
            return _plain_table(header, rows, ".2f")
        return tabulate(rows, headers=header, tablefmt="psql", floatfmt=".2f")

    def save_table(self, filename):
        header = ("overall acc", "overall iou") + self.class_names
        row = [float(self.overall_acc), float(self.overall_iou)] + [float(v) for v in self.class_iou]
        try:
            from tabulate import tabulate
            text = tabulate([row], headers=header, tablefmt="tsv", floatfmt=".5f", numalign=None, stralign=None)
        except ImportError:
            text = "\t".join(header) + "\n" + "\t".join(f"{v:.5f}" for v in row)
        with open(filename, "w") as f:
            f.write(text)


def _i64(x, dev):
    """Labels / predictions -> contiguous (n,) int64 on `dev` (device tensors: no sync)."""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1)).astype(np.int64, copy=False))
    return x.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()


def _logits(x, dev):
    x = x.to(device=dev, dtype=torch.float32)
    if x.dim() != 2:
        raise ValueError(f"evaluate_batch: logits must be (N, C), got {tuple(x.shape)}")
    return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


def evaluate_batch(logit_2d: torch.Tensor, logit_3d: torch.Tensor | None, label: torch.Tensor, evaluators: dict | None = None,
                   pselab: bool = False) -> dict:
    """The metric block of validate() for one batch (validate.py:112-124,126-131,140-170,184-185) as one kernel pass.

    logit_2d / logit_3d: (N, C) per-point logits (any row stride); logit_3d None = the 2D-only path (``model_3d=None``).
    label: (N,) the batch's ``seg_label`` (-100 = ignore): the ground truth of the matrices and of the CE losses.
    evaluators: any subset of {"2D", "3D", "2D+3D", "2D+3D_ety"} -> Evaluator (all with the same classes and labels); each
    gets its predictions of this batch added.  "2D+3D" is the argmax of softmax(l2) + softmax(l3); "2D+3D_ety" the
    entropy-weighted fusion of validate.py:126-131 (weights exp(-sum_c prob_2_entropy(p)), normalised over the two modalities)
    -- a branch the reference itself cannot reach (``entropy_fuse`` is undefined there: NameError at validate.py:125).

    Returns 0-d fp32 device tensors (no host sync): ``val_2d_ety`` / ``val_3d_ety`` = mean(prob_2_entropy(softmax(softmax(l))))
    over all N * C elements (softmax applied to probabilities, as the reference does), ``seg_loss_2d`` / ``seg_loss_3d`` =
    F.cross_entropy(l, label) (NaN when every label is ignored); the 3D entries are None without logit_3d.  ``pselab=True``
    adds ``out["pselab"]``: (N,) device tensors ``pseudo_label_2d`` / ``pseudo_label_3d`` (uint8 argmax) and ``probs_2d`` /
    ``probs_3d`` (softmax at it), the caller splits them per scan (validate.py:159-170).
    """
    dev = logit_2d.device if logit_2d.is_cuda else torch.device("cuda", torch.cuda.current_device())
    l2 = _logits(logit_2d, dev)
    l3 = None if logit_3d is None else _logits(logit_3d, dev)
    n, c = l2.shape
    if l3 is not None and tuple(l3.shape) != (n, c):
        raise ValueError(f"evaluate_batch: logit_3d {tuple(l3.shape)} != logit_2d {(n, c)}")
    if not 1 < c <= MAXC:
        raise ValueError(f"evaluate_batch: {c} classes; the kernel takes 2..{MAXC}")
    if n >= 1 << 31:
        raise ValueError("evaluate_batch: at most 2^31 - 1 points per call")
    lab = _i64(label, dev)
    if lab.numel() != n:
        raise ValueError(f"evaluate_batch: {lab.numel()} labels for {n} points")
    evaluators = dict(evaluators or {})
    unknown = set(evaluators) - set(KINDS)
    if unknown:
        raise ValueError(f"evaluate_batch: unknown evaluator keys {sorted(unknown)}; known: {KINDS}")
    if l3 is None and set(evaluators) - {"2D"}:
        raise ValueError("evaluate_batch: the 3D / xM evaluators need logit_3d")
    evs = list(evaluators.values())
    if any(not evs[0].same_table(e) for e in evs[1:]):
        raise ValueError("evaluate_batch: all evaluators must have the same classes and labels")
    ref = evs[0] if evs else None
    n_labels = ref.num_classes if ref else c
    lut = ref._lut_on(dev) if ref else None
    conf = [evaluators[k]._matrix(dev) if k in evaluators else None for k in KINDS]
    nmod = 1 if l3 is None else 2
    scalars = torch.empty(4, dtype=torch.float32, device=dev)
    ps_pred = torch.empty(nmod, n, dtype=torch.uint8, device=dev) if pselab else None
    ps_prob = torch.empty(nmod, n, dtype=torch.float32, device=dev) if pselab else None
    if n:
        ws = workspace.get(query("mopa_eval_logits_workspace_bytes", n, c), dev)
        call("mopa_eval_logits", ptr(l2), l2.stride(0), ptr(l3), 0 if l3 is None else l3.stride(0), ptr(lab), n, c, ptr(lut),
             0 if lut is None else lut.numel(), n_labels, *[ptr(m) for m in conf], ptr(scalars), ptr(ps_pred), ptr(ps_prob),
             ptr(ws), ws.numel(), stream())
    else:
        scalars.fill_(float("nan"))
    out = {"val_2d_ety": scalars[0], "seg_loss_2d": scalars[2],
           "val_3d_ety": None if l3 is None else scalars[1], "seg_loss_3d": None if l3 is None else scalars[3]}
    if pselab:
        out["pselab"] = {"pseudo_label_2d": ps_pred[0], "probs_2d": ps_prob[0],
                         "pseudo_label_3d": None if l3 is None else ps_pred[1], "probs_3d": None if l3 is None else ps_prob[1]}
    return out
