"""Evaluator's host side (mopa_amd/evaluate.py): derived metrics from the reference Evaluator's own matrices (fixture G9, NaN
quirks included), the table printers without tabulate, and all_reduce over a world-2 gloo group.  No GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


@pytest.fixture(scope="module")
def g9(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g9_evaluator.npz")))


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_derived_metrics_match_reference_evaluator(g9, case):
    from mopa_amd.evaluate import Evaluator
    ev = Evaluator(g9["names"], labels=g9.get(case + "_labels"))
    ev.confusion_matrix = g9[case + "_conf"]
    assert ev.confusion_matrix.dtype == np.float64 and np.array_equal(ev.confusion_matrix, g9[case + "_conf"])
    np.testing.assert_array_equal(np.asarray(ev.class_iou), g9[case + "_class_iou"])          # NaN where union == 0
    np.testing.assert_array_equal(np.asarray(ev.class_seg_acc), g9[case + "_class_seg_acc"])  # NaN where a row is empty
    assert ev.overall_acc == g9[case + "_overall_acc"]
    assert ev.overall_iou == g9[case + "_overall_iou"]          # NaN IoU counted as 0, mean over ALL classes


def test_nan_paths_are_exercised(g9):
    assert np.isnan(g9["a_class_iou"][3]) and np.isnan(g9["a_class_seg_acc"][3])
    from mopa_amd.evaluate import Evaluator
    ev = Evaluator(["x", "y"])
    assert np.isnan(ev.overall_acc) and ev.overall_iou == 0.0 and all(np.isnan(ev.class_iou))


def test_labels_argument_is_checked():
    from mopa_amd.evaluate import Evaluator
    with pytest.raises(ValueError):
        Evaluator(["a", "b"], labels=[0, 1, 2])
    with pytest.raises(ValueError):
        Evaluator(["a", "b"], labels=[0, -1])
    with pytest.raises(ValueError):
        Evaluator([str(i) for i in range(65)])
    ev = Evaluator(["a", "b", "c"], labels=[2, 0, 2])     # sklearn keeps the LAST index of a repeated label
    assert ev._lut_host.tolist() == [1, -1, 2]


def test_print_and_save_table_without_tabulate(g9, monkeypatch, tmp_path):
    from mopa_amd.evaluate import Evaluator
    ev = Evaluator(g9["names"])
    ev.confusion_matrix = g9["a_conf"]
    monkeypatch.setitem(sys.modules, "tabulate", None)       # `from tabulate import tabulate` raises ImportError
    text = ev.print_table()
    lines = text.splitlines()
    assert [c.strip() for c in lines[1].strip("|").split("|")] == ["Class", "Accuracy", "IOU", "Total"]
    rows = [[c.strip() for c in ln.strip("|").split("|")] for ln in lines[3:-1]]
    assert [r[0] for r in rows] == list(g9["names"])
    acc, iou = g9["a_class_seg_acc"] * 100, g9["a_class_iou"] * 100
    for i, r in enumerate(rows):
        assert r[1] == f"{acc[i]:.2f}" and r[2] == f"{iou[i]:.2f}" and r[3] == str(int(g9["a_conf"][i].sum()))
    assert rows[3][1] == "nan" and rows[3][2] == "nan"
    ev.save_table(tmp_path / "t.tsv")
    head, vals = (tmp_path / "t.tsv").read_text().splitlines()
    assert head.split("\t") == ["overall acc", "overall iou"] + list(g9["names"])
    assert vals.split("\t")[:2] == [f"{g9['a_overall_acc']:.5f}", f"{g9['a_overall_iou']:.5f}"]


def test_print_table_with_tabulate_has_the_same_cells(g9):
    pytest.importorskip("tabulate")
    from mopa_amd.evaluate import Evaluator
    ev = Evaluator(g9["names"])
    ev.confusion_matrix = g9["a_conf"]
    text = ev.print_table()
    assert "Accuracy" in text and all(name in text for name in g9["names"])
    assert f"{g9['a_class_iou'][0] * 100:.2f}" in text


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mopa_amd.evaluate import Evaluator
    mats = [np.arange(9).reshape(3, 3) * (r + 1) + 10 ** 12 for r in range(world)]   # beyond fp32 / fp64-exact-sum doubt
    ev = Evaluator(["a", "b", "c"])
    ev.confusion_matrix = mats[rank]
    ev.all_reduce()
    empty = Evaluator(["a", "b", "c"])
    empty.all_reduce()
    q.put((rank, ev._conf.numpy().tolist(), empty.confusion_matrix.tolist()))
    dist.destroy_process_group()


def test_all_reduce_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want = (np.arange(9).reshape(3, 3) * 3 + 2 * 10 ** 12).tolist()
    for rank, got, empty in res:
        assert got == want and empty == np.zeros((3, 3)).tolist(), rank
