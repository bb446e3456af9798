"""Host side of the fused training-loss block (mopa_amd/trainloss.py): the ABI names, the CPU refusal and SegIoU.add_matrix."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mopa_point_losses_workspace_bytes", "mopa_point_losses_fwd", "mopa_point_losses_bwd")


def test_entry_points_are_declared():
    from mopa_amd import _abi
    header = open(os.path.join(ROOT, "include", "mopa_hip.h")).read()
    for name in NAMES:
        assert name in _abi.SIGNATURES
        assert name + "(" in header
    assert _abi.SIGNATURES["mopa_point_losses_workspace_bytes"] == ("z", "l")
    assert _abi.SIGNATURES["mopa_point_losses_fwd"][1].endswith("pzp") and _abi.SIGNATURES["mopa_point_losses_bwd"][1].endswith("p")
    assert not any(n in _abi.HOST_PARAMS for n in NAMES)   # device pointers only


def test_point_losses_refuses_cpu_tensors():
    from mopa_amd.trainloss import point_losses
    z = torch.randn(7, 5, requires_grad=True)
    with pytest.raises(RuntimeError):
        point_losses({"seg_logit": z}, {"seg_logit": z.detach().clone()}, label=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        point_losses(None, {"seg_logit": z, "seg_logit2": z + 1}, label_3d=torch.zeros(7, dtype=torch.int64))


def _case(seed, n=500, C=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    logit = torch.from_numpy(rng.standard_normal((n, C), dtype=np.float32) * 2)
    label = rng.integers(0, C, n)
    label[rng.random(n) < 0.3] = -100
    assert (label == -100).any()
    return logit, torch.from_numpy(label)


def _matrix(logit, label, C):
    mat = np.zeros((C, C), np.int64)
    keep = label.numpy() != -100
    np.add.at(mat, (label.numpy()[keep], logit.numpy().argmax(1)[keep]), 1)
    return torch.from_numpy(mat)


def test_add_matrix_equals_update_dict():
    from mopa_amd.models.metric import SegIoU
    C = 5
    a, b = SegIoU(C), SegIoU(C)
    for seed in (1, 2, 3):
        logit, label = _case(seed, C=C)
        a.update_dict({"seg_logit": logit}, {"seg_label": label})
        b.add_matrix(_matrix(logit, label, C))
        assert b.mat.dtype == torch.int64 and torch.equal(a.mat, b.mat)
    assert torch.equal(a.iou, b.iou) and a.global_avg == b.global_avg
    b.reset()
    assert b.mat is None


def test_update_dict_after_add_matrix_still_accumulates():
    from mopa_amd.models.metric import SegIoU
    C = 5
    (l1, y1), (l2, y2) = _case(11, C=C), _case(12, C=C)
    m = SegIoU(C)
    first = _matrix(l1, y1, C)
    m.add_matrix(first)
    m.update_dict({"seg_logit": l2}, {"seg_label": y2})
    assert torch.equal(m.mat, _matrix(l1, y1, C) + _matrix(l2, y2, C))
    assert torch.equal(first, _matrix(l1, y1, C))            # the matrix handed in is not written
    m.add_matrix(_matrix(l1, y1, C))
    assert int(m.mat.sum()) == 2 * int((y1 != -100).sum()) + int((y2 != -100).sum())


def test_add_matrix_refuses_other_shapes_and_types():
    from mopa_amd.models.metric import SegIoU
    m = SegIoU(5)
    with pytest.raises(ValueError):
        m.add_matrix(torch.zeros(4, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        m.add_matrix(torch.zeros(5, 5, dtype=torch.int32))
    assert m.mat is None
