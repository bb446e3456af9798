"""Host side of the merged-pass loss block (mopa_amd/trainloss.py::point_losses_merged): the ABI names, the descriptor as the only
host pointer, and the refusals that come before anything is launched."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mopa_point_losses_seg_workspace_bytes", "mopa_point_losses_seg_fwd", "mopa_point_losses_seg_bwd")


def test_entry_points_are_declared():
    from mopa_amd import _abi
    header = open(os.path.join(ROOT, "include", "mopa_hip.h")).read()
    for name in NAMES:
        assert name in _abi.SIGNATURES
        assert name + "(" in header
    assert _abi.SIGNATURES["mopa_point_losses_seg_workspace_bytes"] == ("z", "i")
    assert _abi.SIGNATURES["mopa_point_losses_seg_fwd"][1].endswith("pzp") and _abi.SIGNATURES["mopa_point_losses_seg_bwd"][1].endswith("p")


def test_only_the_descriptor_is_a_host_pointer():
    from mopa_amd import _abi
    assert "mopa_point_losses_seg_workspace_bytes" not in _abi.HOST_PARAMS
    for name in NAMES[1:]:
        host = _abi.HOST_PARAMS[name]
        assert list(host.values()) == ["segs_host"]
        (at,) = host
        assert _abi.SIGNATURES[name][1][at] == "p" and _abi.SIGNATURES[name][1][at + 1] == "i"     # the table, then S
    # the existing block keeps device pointers only
    assert not any(n in _abi.HOST_PARAMS for n in ("mopa_point_losses_fwd", "mopa_point_losses_bwd"))


def test_workspace_query_runs_on_the_host():
    from mopa_amd import _lib
    one, eight = _lib.query("mopa_point_losses_seg_workspace_bytes", 1), _lib.query("mopa_point_losses_seg_workspace_bytes", 8)
    assert one >= 8 * 2048 * 8 and eight >= 8 * one - 8 * 256


def _preds(n2, n3, C=5):
    p2 = None if n2 is None else {"seg_logit": torch.randn(n2, C, requires_grad=True)}
    p3 = None if n3 is None else {"seg_logit": torch.randn(n3, C, requires_grad=True)}
    return p2, p3


def test_refusals_before_any_launch(monkeypatch):
    from mopa_amd import trainloss
    from mopa_amd.trainloss import Segment, point_losses_merged
    calls = []
    monkeypatch.setattr(trainloss, "call", lambda name, *a: calls.append(name))
    y = torch.zeros(7, dtype=torch.int64)
    # CPU tensors
    p2, p3 = _preds(14, 14)
    with pytest.raises(RuntimeError, match="CPU"):
        point_losses_merged(p2, p3, [Segment(7, label=y), Segment(7, label=y)])
    with pytest.raises(RuntimeError, match="CPU"):
        point_losses_merged(None, p3, [Segment(14, label_3d=torch.zeros(14, dtype=torch.int64))])
    # row counts that do not add up to the logits' rows: in both networks, in the 3D network alone (a third, 3D-only segment missing)
    with pytest.raises(ValueError, match="rows"):
        point_losses_merged(p2, p3, [Segment(7, label=y), Segment(6, label=y)])
    p2, p3 = _preds(14, 21)
    with pytest.raises(ValueError, match="3D segments hold 14 rows, the logits 21"):
        point_losses_merged(p2, p3, [Segment(7, label=y), Segment(7, label=y)])
    with pytest.raises(ValueError, match="2D segments hold 21 rows, the logits 14"):
        point_losses_merged(p2, p3, [Segment(7, label=y), Segment(7, label=y), Segment(7, label_3d=y)])     # in_2d left on
    with pytest.raises(RuntimeError, match="CPU"):                                                          # ... and the right form
        point_losses_merged(p2, p3, [Segment(7, label=y), Segment(7, label=y), Segment(7, label_3d=y, in_2d=False)])
    # 9 segments, none
    p2, p3 = _preds(9, 9)
    with pytest.raises(ValueError, match="9 segments"):
        point_losses_merged(p2, p3, [Segment(1) for _ in range(9)])
    with pytest.raises(ValueError, match="0 segments"):
        point_losses_merged(p2, p3, [])
    # minent with one class
    p2, p3 = _preds(7, 7, C=1)
    with pytest.raises(ValueError, match="two classes"):
        point_losses_merged(p2, p3, [Segment(7, minent=True)])
    with pytest.raises(ValueError):
        point_losses_merged(None, None, [Segment(7)])
    assert calls == []


def test_segment_defaults():
    from mopa_amd.trainloss import MAX_SEGMENTS, Segment
    s = Segment(5)
    assert (s.rows, s.weighted, s.kl, s.minent, s.in_2d, s.in_3d) == (5, True, True, False, True, True)
    assert s.label is None and s.label_2d is None and s.label_3d is None and s.metric_2d is None and s.metric_3d is None and s.acc_mask is None
    assert MAX_SEGMENTS == 8
