"""Validation metrics on the device (mopa_amd/evaluate.py, csrc/evaluate.hip) against the reference Evaluator (fixture G9), a
numpy restatement of it, and torch's composition of validate.py:112-124,184-185."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.pseudo import prob_2_entropy

pytestmark = pytest.mark.gpu


def np_confusion(pred, gt, L, labels=None):
    """evaluate.py:12-26 restated: ground truth -100 -> L, then sklearn's labels= (values not listed are dropped), rows = gt."""
    pred, gt = np.asarray(pred, np.int64).ravel(), np.asarray(gt, np.int64).ravel()
    gt = np.where(gt == -100, L, gt)
    labels = np.arange(L) if labels is None else np.asarray(labels)
    lut = np.full(max(int(labels.max()), int(max(pred.max(initial=0), gt.max(initial=0)))) + 1, -1)
    lut[labels] = np.arange(L)

    def idx(v):
        out = np.full(v.shape, -1)
        ok = v >= 0
        out[ok] = lut[v[ok]]
        return out
    gi, pi = idx(gt), idx(pred)
    keep = (gi >= 0) & (pi >= 0)
    return np.bincount(gi[keep] * L + pi[keep], minlength=L * L).reshape(L, L).astype(np.float64)


def torch_ref(l2, l3, label):
    """validate.py:112-124,184-185 on the same logits: predictions (fp32, device), entropy means and CE in fp64."""
    p2, p3 = F.softmax(l2, 1), F.softmax(l3, 1)
    s = p2 + p3
    top = s.topk(2, 1).values
    near = (top[:, 0] - top[:, 1]) <= 4 * torch.finfo(torch.float32).eps * top[:, 0]    # within ~4 ulp: rounding decides
    d2, d3 = l2.double(), l3.double()
    # labels outside [0, C) other than -100 are skipped by the kernel; torch's CE would index out of bounds
    label = torch.where((label >= 0) & (label < l2.shape[1]), label, torch.full_like(label, -100))
    return dict(pred_2d=l2.argmax(1), pred_3d=l3.argmax(1), pred_xm=s.argmax(1), near=near,
                ety_2d=prob_2_entropy(F.softmax(F.softmax(d2, 1), 1)).mean().item(),
                ety_3d=prob_2_entropy(F.softmax(F.softmax(d3, 1), 1)).mean().item(),
                ce_2d=F.cross_entropy(d2, label).item(), ce_3d=F.cross_entropy(d3, label).item())


def check_xm(got, pred_xm, near, label, L, labels=None):
    """xM matrix == the torch prediction's except at near-ties (each moves at most one count out of a cell and into another)."""
    ref = np_confusion(pred_xm.cpu().numpy(), label.cpu().numpy(), L, labels)
    n_near = int(near.sum())
    assert n_near <= max(1, 1e-4 * near.numel()), n_near
    assert np.abs(got - ref).sum() <= 2 * n_near


def make(n, c, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    l2 = torch.randn(n, c, generator=g) * scale
    l3 = torch.randn(n, c, generator=g) * scale
    label = torch.randint(0, c, (n,), generator=g)
    label[torch.rand(n, generator=g) < 0.1] = -100
    label[torch.rand(n, generator=g) < 0.01] = c + 3          # outside [0, C): no CE term, dropped from the matrices
    return l2.cuda(), l3.cuda(), label.cuda()


def run(l2, l3, label, names, labels=None, kinds=("2D", "3D", "2D+3D"), **kw):
    from mopa_amd.evaluate import Evaluator, evaluate_batch
    evs = {k: Evaluator(names, labels) for k in kinds}
    out = evaluate_batch(l2, l3, label, evaluators=evs, **kw)
    return evs, out


# ------------------------------------------------------------------------------------------------ 1, 2, 3
@pytest.mark.parametrize("c,n", [(5, 1), (5, 1000), (10, 257), (11, 100_003), (64, 4099), (5, 32 * 120_000)])
def test_matrices_predictions_and_scalars(c, n):
    names = [f"c{i}" for i in range(c)]
    l2, l3, label = make(n, c, seed=n + c)
    evs, out = run(l2, l3, label, names, pselab=True)
    ref = torch_ref(l2, l3, label)
    lab = label.cpu().numpy()
    p2, p3 = out["pselab"]["pseudo_label_2d"], out["pselab"]["pseudo_label_3d"]
    assert torch.equal(p2.long(), ref["pred_2d"]) and torch.equal(p3.long(), ref["pred_3d"])
    assert np.array_equal(evs["2D"].confusion_matrix, np_confusion(ref["pred_2d"].cpu().numpy(), lab, c))
    assert np.array_equal(evs["3D"].confusion_matrix, np_confusion(ref["pred_3d"].cpu().numpy(), lab, c))
    check_xm(evs["2D+3D"].confusion_matrix, ref["pred_xm"], ref["near"], label, c)
    for key, r in (("val_2d_ety", ref["ety_2d"]), ("val_3d_ety", ref["ety_3d"]), ("seg_loss_2d", ref["ce_2d"]), ("seg_loss_3d", ref["ce_3d"])):
        assert out[key].dim() == 0 and out[key].is_cuda
        np.testing.assert_allclose(out[key].item(), r, rtol=1e-5, err_msg=key)


def test_custom_labels_order_and_out_of_range_values():
    c = 10
    names = [f"c{i}" for i in range(c)]
    labels = [7, 3, 0, 9, 1, 2, 8, 4, 6, 10]                   # 10 == num_classes: the reference counts -100 ground truth there
    l2, l3, label = make(50_001, c, seed=4)
    evs, out = run(l2, l3, label, names, labels)
    ref = torch_ref(l2, l3, label)
    lab = label.cpu().numpy()
    assert np.array_equal(evs["2D"].confusion_matrix, np_confusion(ref["pred_2d"].cpu().numpy(), lab, c, labels))
    assert np.array_equal(evs["3D"].confusion_matrix, np_confusion(ref["pred_3d"].cpu().numpy(), lab, c, labels))
    counted = (lab == -100) & (ref["pred_2d"].cpu().numpy() != 5)        # class 5 is not in labels: dropped as a prediction
    assert evs["2D"].confusion_matrix[:, -1].sum() == 0 and evs["2D"].confusion_matrix[-1].sum() == counted.sum() > 0
    check_xm(evs["2D+3D"].confusion_matrix, ref["pred_xm"], ref["near"], label, c, labels)
    # Evaluator.update(pred, gt) with predictions outside [0, C) and the same labels
    from mopa_amd.evaluate import Evaluator
    pred = torch.randint(-3, c + 3, (50_001,), generator=torch.Generator().manual_seed(1))
    ev = Evaluator(names, labels)
    ev.update(pred.cuda(), label)
    assert np.array_equal(ev.confusion_matrix, np_confusion(pred.numpy(), lab, c, labels))


def test_reference_evaluator_golden(golden_dir):
    from mopa_amd.evaluate import Evaluator, evaluate_batch
    g = dict(np.load(os.path.join(golden_dir, "g9_evaluator.npz")))
    for case in ("a", "b", "c"):
        ev = Evaluator(g["names"], g.get(case + "_labels"))
        gt = g[case + "_gt"].copy()
        ev.batch_update(np.split(g[case + "_pred"], np.cumsum(g[case + "_len"])[:-1]), np.split(gt, np.cumsum(g[case + "_len"])[:-1]))
        assert np.array_equal(gt, g[case + "_gt"])             # documented deviation: the caller's labels are not rewritten
        assert np.array_equal(ev.confusion_matrix, g[case + "_conf"]), case
        np.testing.assert_array_equal(np.asarray(ev.class_iou), g[case + "_class_iou"])
        assert ev.overall_iou == g[case + "_overall_iou"]
    l2, l3, label = (torch.from_numpy(g[k]).cuda() for k in ("l_logit_2d", "l_logit_3d", "l_label"))
    evs = {k: Evaluator(g["names"]) for k in ("2D", "3D", "2D+3D")}
    out = evaluate_batch(l2, l3, label, evaluators=evs)
    assert np.array_equal(evs["2D"].confusion_matrix, g["l_conf_2d"]) and np.array_equal(evs["3D"].confusion_matrix, g["l_conf_3d"])
    assert np.abs(evs["2D+3D"].confusion_matrix - g["l_conf_xm"]).sum() <= 2 * int(torch_ref(l2, l3, label)["near"].sum())
    np.testing.assert_allclose(out["val_2d_ety"].item(), g["l_ety_2d_f64"], rtol=1e-5)
    np.testing.assert_allclose(out["val_3d_ety"].item(), g["l_ety_3d_f64"], rtol=1e-5)
    np.testing.assert_allclose(out["seg_loss_2d"].item(), g["l_ce_2d"], rtol=1e-5)
    np.testing.assert_allclose(out["seg_loss_3d"].item(), g["l_ce_3d"], rtol=1e-5)


def test_ce_is_nan_when_every_label_is_ignored_and_2d_only_path():
    l2, l3, label = make(3000, 5, seed=2)
    ignored = torch.full((3000,), -100, dtype=torch.int64, device="cuda")
    _, out = run(l2, l3, ignored, list("abcde"))
    assert torch.isnan(out["seg_loss_2d"]) and torch.isnan(out["seg_loss_3d"]) and torch.isfinite(out["val_2d_ety"])
    from mopa_amd.evaluate import Evaluator, evaluate_batch
    ev = Evaluator(list("abcde"))
    out = evaluate_batch(l2, None, label, evaluators={"2D": ev})
    assert out["val_3d_ety"] is None and out["seg_loss_3d"] is None and torch.isfinite(out["seg_loss_2d"])
    ref = torch_ref(l2, l3, label)
    np.testing.assert_allclose(out["seg_loss_2d"].item(), ref["ce_2d"], rtol=1e-5)
    assert np.array_equal(ev.confusion_matrix, np_confusion(ref["pred_2d"].cpu().numpy(), label.cpu().numpy(), 5))
    with pytest.raises(ValueError):
        evaluate_batch(l2, None, label, evaluators={"3D": Evaluator(list("abcde"))})


def test_strided_logits_take_the_unstaged_path():
    """A channel slice of a wider buffer (row stride > C) and a non-contiguous label: same results as contiguous copies."""
    wide2, wide3, label = make(20_000, 12, seed=5)
    l2, l3 = wide2[:, 2:7], wide3[:, 5:10]
    evs_a, out_a = run(l2, l3, label, list("abcde"), kinds=("2D", "3D", "2D+3D", "2D+3D_ety"))
    evs_b, out_b = run(l2.contiguous(), l3.contiguous(), label, list("abcde"), kinds=("2D", "3D", "2D+3D", "2D+3D_ety"))
    for k in evs_a:
        assert np.array_equal(evs_a[k].confusion_matrix, evs_b[k].confusion_matrix), k
    for k in ("val_2d_ety", "val_3d_ety", "seg_loss_2d", "seg_loss_3d"):
        np.testing.assert_allclose(out_a[k].item(), out_b[k].item(), rtol=1e-6)


def test_entropy_fused_prediction():
    """validate.py:126-131 restated in torch (fp32): matrix equal except at near-ties."""
    l2, l3, label = make(40_000, 5, seed=6)
    evs, _ = run(l2, l3, label, list("abcde"), kinds=("2D+3D_ety",))
    p2, p3 = F.softmax(l2, 1), F.softmax(l3, 1)
    r2, r3 = torch.exp(-prob_2_entropy(p2).sum(1)), torch.exp(-prob_2_entropy(p3).sum(1))
    fused = (r2 / (r2 + r3)).unsqueeze(1) * p2 + (r3 / (r2 + r3)).unsqueeze(1) * p3
    top = fused.topk(2, 1).values
    near = (top[:, 0] - top[:, 1]) <= 8 * torch.finfo(torch.float32).eps * top[:, 0]
    ref = np_confusion(fused.argmax(1).cpu().numpy(), label.cpu().numpy(), 5)
    assert int(near.sum()) <= 4 and np.abs(evs["2D+3D_ety"].confusion_matrix - ref).sum() <= 2 * int(near.sum())


# ------------------------------------------------------------------------------------------------ 4, 5, 6, 7
def test_two_calls_are_bit_identical():
    l2, l3, label = make(1_000_003, 10, seed=7)
    names = [str(i) for i in range(10)]
    kinds = ("2D", "3D", "2D+3D", "2D+3D_ety")
    evs_a, a = run(l2, l3, label, names, kinds=kinds, pselab=True)
    evs_b, b = run(l2, l3, label, names, kinds=kinds, pselab=True)
    for k in kinds:
        assert torch.equal(evs_a[k]._conf, evs_b[k]._conf)
    for k in ("val_2d_ety", "val_3d_ety", "seg_loss_2d", "seg_loss_3d"):
        assert torch.equal(a[k], b[k])
    for k, v in a["pselab"].items():
        assert torch.equal(v, b["pselab"][k])


def test_one_call_over_32_scans_equals_per_scan_calls_and_update():
    from mopa_amd.evaluate import Evaluator, evaluate_batch
    rng = np.random.Generator(np.random.PCG64(8))
    lens = rng.integers(1, 40_000, 32)
    n = int(lens.sum())
    l2, l3, label = make(n, 5, seed=8)
    names = list("abcde")
    evs, _ = run(l2, l3, label, names)
    per = {k: Evaluator(names) for k in evs}
    upd = {k: Evaluator(names) for k in ("2D", "3D")}
    left = 0
    for m in lens:
        sl = slice(left, left + int(m))
        o = evaluate_batch(l2[sl], l3[sl], label[sl], evaluators=per, pselab=True)
        upd["2D"].update(o["pselab"]["pseudo_label_2d"], label[sl])
        upd["3D"].update(o["pselab"]["pseudo_label_3d"], label[sl])
        left += int(m)
    for k in evs:
        assert torch.equal(evs[k]._conf, per[k]._conf), k
    for k in upd:
        assert torch.equal(evs[k]._conf, upd[k]._conf), k


def test_no_host_sync_with_device_inputs():
    from mopa_amd.evaluate import Evaluator, evaluate_batch
    l2, l3, label = make(100_000, 10, seed=9)
    names = [str(i) for i in range(10)]
    evs = {k: Evaluator(names, labels=list(range(9, -1, -1))) for k in ("2D", "3D", "2D+3D", "2D+3D_ety")}
    pred = l2.argmax(1)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = evaluate_batch(l2, l3, label, evaluators=evs, pselab=True)
        evs["2D"].update(pred, label)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.cuda.get_sync_debug_mode() == prev
    assert evs["2D"].confusion_matrix.sum() == 2 * evs["3D"].confusion_matrix.sum() and torch.isfinite(out["seg_loss_2d"])


def test_pselab_outputs_equal_softmax_gather_at_argmax():
    l2, l3, label = make(120_000, 10, seed=10)
    _, out = run(l2, l3, label, [str(i) for i in range(10)], pselab=True)
    ps = out["pselab"]
    for tag, lg in (("2d", l2), ("3d", l3)):
        pred = lg.argmax(1)
        assert ps["pseudo_label_" + tag].dtype == torch.uint8 and torch.equal(ps["pseudo_label_" + tag].long(), pred)
        want = F.softmax(lg, 1)[torch.arange(lg.shape[0], device="cuda"), pred]
        torch.testing.assert_close(ps["probs_" + tag], want, rtol=2e-6, atol=0)


def test_bad_arguments_are_refused():
    from mopa_amd._lib import call
    from mopa_amd.evaluate import Evaluator, evaluate_batch
    l2, l3, label = make(100, 65, seed=11)
    with pytest.raises(ValueError):
        evaluate_batch(l2, l3, label)
    with pytest.raises(RuntimeError):
        call("mopa_confusion_update", label.data_ptr(), label.data_ptr(), 100, None, 0, 65, label.data_ptr(), 0)
    with pytest.raises(ValueError):
        Evaluator(list("ab")).update(np.zeros(3, np.int64), np.zeros(4, np.int64))


# ------------------------------------------------------------------------------------------------ 8: full-size runs
def _models(num_classes):
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d, build_model_3d
    torch.manual_seed(0)
    cfg = default_cfg(num_classes=num_classes)
    return build_model_2d(cfg)[0].cuda().eval(), build_model_3d(cfg)[0].cuda().eval()


def _full_size(batch, num_classes, pselab):
    from mopa_amd.evaluate import Evaluator, evaluate_batch
    m2, m3 = _models(num_classes)
    batch["img"] = batch["img"].cuda()
    with torch.no_grad():
        l2 = m2(batch)["seg_logit"]                           # one call per network
        l3 = m3(batch)["seg_logit"]
    label = batch["seg_label"].cuda()
    assert torch.isfinite(l2).all() and torch.isfinite(l3).all()
    names = [str(i) for i in range(num_classes)]
    evs = {k: Evaluator(names) for k in ("2D", "3D", "2D+3D")}
    out = evaluate_batch(l2, l3, label, evaluators=evs, pselab=pselab)
    ref = torch_ref(l2, l3, label)
    lab = label.cpu().numpy()
    assert np.array_equal(evs["2D"].confusion_matrix, np_confusion(ref["pred_2d"].cpu().numpy(), lab, num_classes))
    assert np.array_equal(evs["3D"].confusion_matrix, np_confusion(ref["pred_3d"].cpu().numpy(), lab, num_classes))
    check_xm(evs["2D+3D"].confusion_matrix, ref["pred_xm"], ref["near"], label, num_classes)
    for key, r in (("val_2d_ety", ref["ety_2d"]), ("val_3d_ety", ref["ety_3d"]), ("seg_loss_2d", ref["ce_2d"]), ("seg_loss_3d", ref["ce_3d"])):
        np.testing.assert_allclose(out[key].item(), r, rtol=1e-5, err_msg=key)
    return l2, l3, out


def test_full_size_32_nuscenes_scans_one_call_per_network():
    from mopa_amd import synth
    batch = synth.make_batch(32, H=225, W=400)
    l2, _, _ = _full_size(batch, 5, pselab=False)
    assert l2.shape == (32 * 34_880, 5)


def test_full_size_kitti_scan_pselab_batch_1():
    from mopa_amd import synth
    batch = synth.make_batch(1, shape=synth.KITTI)
    l2, l3, out = _full_size(batch, 10, pselab=True)
    assert l2.shape == (120_000, 10)
    ps = out["pselab"]
    for tag, lg in (("2d", l2), ("3d", l3)):
        pred = lg.argmax(1)
        assert torch.equal(ps["pseudo_label_" + tag].long(), pred)
        torch.testing.assert_close(ps["probs_" + tag], F.softmax(lg, 1)[torch.arange(lg.shape[0], device="cuda"), pred], rtol=2e-6, atol=0)
