"""Generate tests/golden/g9_evaluator.npz by RUNNING THE REFERENCE's own ``Evaluator`` (mopa/data/utils/evaluate.py, sklearn
confusion_matrix) and ``prob_2_entropy`` (mopa/models/losses.py:10-19) on small synthetic inputs, on the host.

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed .npz is what travels).
Usage, from the repo root:  python tests/golden_gen/g9_evaluator.py PATH_TO_MOPA_CHECKOUT
The reference's Python is imported, never copied.  ``mopa.models.xmuda_arch`` (imported by losses.py for an unrelated helper) is
stubbed: its network code needs packages that are not installed and plays no part in prob_2_entropy.

Cases (prefix in the .npz):
  a_*  5 classes, 3 scans: -100 ground truth, a class absent from ground truth AND predictions (NaN accuracy / IoU paths).
  b_*  custom labels= order [4, 2, 0, 1, 3]; values outside labels (7, 9) in predictions and ground truth are dropped.
  c_*  labels=[3, 1, 5, 0, 2]: 5 == num_classes, so the reference's -100 -> num_classes rewrite COUNTS ignored points (row 2).
  l_*  logits: 2000 points x 5 classes in 4 scans, integer-valued logits (many exact ties), 10 % -100 labels; the reference's
       validate() composition (validate.py:112-124,184): argmax predictions, softmax-sum xM prediction, per-scan Evaluator
       updates, entropy means, CE.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "g9_evaluator.npz")


def _load(ref):
    spec = importlib.util.spec_from_file_location("ref_evaluate", os.path.join(ref, "mopa", "data", "utils", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    stub = types.ModuleType("mopa.models.xmuda_arch")
    stub.batch_segment = None
    sys.modules["mopa.models.xmuda_arch"] = stub
    sys.path.insert(0, ref)
    from mopa.models.losses import prob_2_entropy  # reference
    return ev.Evaluator, prob_2_entropy


def _metrics(out, key, ev):
    out[key + "_conf"] = ev.confusion_matrix.copy()
    out[key + "_overall_acc"] = np.float64(ev.overall_acc)
    out[key + "_overall_iou"] = np.float64(ev.overall_iou)
    out[key + "_class_seg_acc"] = np.asarray(ev.class_seg_acc, np.float64)
    out[key + "_class_iou"] = np.asarray(ev.class_iou, np.float64)


def main(ref):
    Evaluator, prob_2_entropy = _load(ref)
    rng = np.random.Generator(np.random.PCG64(9))
    out = {}
    names = np.array(["car", "truck", "bike", "person", "vegetation"])
    out["names"] = names

    # a: default labels; class 3 never appears
    ev = Evaluator(names)
    preds, gts = [], []
    for n in (50, 1, 333):
        gt = rng.choice([0, 1, 2, 4], n)
        gt[rng.random(n) < 0.2] = -100
        if n == 1:
            gt[0] = 2
        pred = rng.choice([0, 1, 2, 4], n)
        preds.append(pred)
        gts.append(gt.copy())
        ev.update(pred, gt)                      # mutates gt: the copy above is the input
    out["a_pred"], out["a_gt"], out["a_len"] = np.concatenate(preds), np.concatenate(gts), np.array([len(p) for p in preds])
    _metrics(out, "a", ev)

    for key, labels in (("b", [4, 2, 0, 1, 3]), ("c", [3, 1, 5, 0, 2])):
        ev = Evaluator(names, labels=labels)
        preds, gts = [], []
        for n in (120, 77):
            gt = rng.choice([0, 1, 2, 3, 4, 5, 7, 9], n)
            gt[rng.random(n) < 0.15] = -100
            pred = rng.choice([0, 1, 2, 3, 4, 5, 7], n)
            preds.append(pred)
            gts.append(gt.copy())
            ev.update(pred, gt)
        out[key + "_labels"] = np.asarray(labels)
        out[key + "_pred"], out[key + "_gt"], out[key + "_len"] = np.concatenate(preds), np.concatenate(gts), np.array([len(p) for p in preds])
        _metrics(out, key, ev)

    # l: logits through the reference's composition
    n, c = 2000, 5
    l2 = torch.from_numpy(rng.integers(-2, 3, (n, c)).astype(np.float32))
    l3 = torch.from_numpy(rng.integers(-2, 3, (n, c)).astype(np.float32) * 0.5)
    label = torch.from_numpy(rng.integers(0, c, n))
    label[torch.from_numpy(rng.random(n) < 0.1)] = -100
    lens = np.array([700, 1, 555, 744])
    p2, p3 = F.softmax(l2, dim=1), F.softmax(l3, dim=1)
    pred2, pred3, predx = l2.argmax(1).numpy(), l3.argmax(1).numpy(), (p2 + p3).argmax(1).numpy()
    evs = {k: Evaluator(names) for k in ("2D", "3D", "2D+3D")}
    left = 0
    for m in lens:
        gt = label[left:left + m].numpy()
        for k, p in (("2D", pred2), ("3D", pred3), ("2D+3D", predx)):
            evs[k].update(p[left:left + m], gt.copy())
        left += m
    out["l_logit_2d"], out["l_logit_3d"], out["l_label"], out["l_len"] = l2.numpy(), l3.numpy(), label.numpy(), lens
    out["l_pred_2d"], out["l_pred_3d"], out["l_pred_xm"] = pred2, pred3, predx
    for k, tag in (("2D", "2d"), ("3D", "3d"), ("2D+3D", "xm")):
        out["l_conf_" + tag] = evs[k].confusion_matrix.copy()
    for tag, lg in (("2d", l2), ("3d", l3)):
        out["l_ety_" + tag] = np.float64(torch.mean(prob_2_entropy(F.softmax(F.softmax(lg, dim=1), dim=1))).item())
        out["l_ety_" + tag + "_f64"] = np.float64(torch.mean(prob_2_entropy(F.softmax(F.softmax(lg.double(), dim=1), dim=1))).item())
        out["l_ce_" + tag] = np.float64(F.cross_entropy(lg.double(), label).item())
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
