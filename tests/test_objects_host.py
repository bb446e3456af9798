"""mopa_amd/objects.py without a GPU: the restatement tests/_objects_reference.py against sklearn on the shared cases, ClusterParams
and the argument checks (which come before any device is touched), and ObjectBank: the cap and its order, the file names and bytes,
the load round trip, and sample against a restated obj_sampling (the same np.random draws)."""
import os

import numpy as np
import pytest
import torch

import _objects_reference as ref

F32 = np.float32


@pytest.fixture(scope="module")
def cases():
    return ref.build_cases()


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_the_restatement_gives_sklearns_labels(cases):
    cluster = pytest.importorskip("sklearn.cluster")
    n_seg = n_pts = 0
    for name, c in cases.items():
        eps, ms = c.get("eps", ref.EPS), c.get("min_samples", ref.MIN_SAMPLES)
        for X in ref.segments(c):
            if len(X) == 0:
                continue                                    # sklearn refuses an empty array; the reference skips such a class
            want = cluster.DBSCAN(eps=eps, min_samples=ms).fit_predict(X)
            assert np.array_equal(ref.dbscan_labels(X, eps, ms), want), name
            n_seg += 1
            n_pts += len(X)
    assert n_seg > 100 and n_pts > 10000


def test_the_cases_test_what_they_are_named_for(cases):
    """The restatement alone, so that a case cannot pass by being empty."""
    ex = lambda name: ref.extract(cases[name]["points"], cases[name]["labels"], cases[name]["class_ids"], **ref.params_of(cases[name]))  # noqa: E731
    assert len(ex("empty scan")["table"]) == 0 and len(ex("no point of a requested class")["table"]) == 0
    assert ex("one point")["table"].tolist() == [[0, 0, -1, 1]] and ex("four points")["table"].tolist() == [[0, 0, -1, 4]]
    assert ex("five coincident points")["table"].tolist() == [[0, 0, 0, 5]]
    assert ex("min_samples and one fewer")["table"].tolist() == [[0, 0, -1, 4], [0, 0, 0, 5]]
    r = ex("ties at eps on a lattice")
    assert r["table"].tolist() == [[0, 0, 0, 27], [0, 1, -1, 27], [0, 2, 0, 6], [0, 3, -1, 6]]
    for name in ("chain, lowest core at the near end", "chain, lowest core in the middle", "chain, lowest core at the far end", "chain, shuffled"):
        r = ex(name)
        assert sorted(r["table"][:, 3].tolist()) == [40, 600] and (r["labels"][0] >= 0).all(), name
    assert ex("chain, lowest core at the far end")["table"][:, 3].tolist() == [40, 600]
    r = ex("a border point between two clusters, last")      # B's rows come first: B is cluster 0 and takes the bridge
    assert r["labels"][0].tolist() == [0] * 5 + [1] * 5 + [0]
    r = ex("a border point between two clusters, first")
    assert r["labels"][0].tolist() == [0] + [0] * 5 + [1] * 5
    assert ex("lowest index is a border point")["labels"][0].tolist() == [1] + [0] * 5 + [1] * 5
    assert ex("a blob inside one cell")["table"].tolist() == [[0, 0, 0, 3000]]
    r = ex("the same points in two scans and two classes")
    assert r["table"].tolist() == [[b, c, i, n] for b in (0, 1) for c in (0, 1) for i, n in ((-1, 3), (0, 5))]
    r = ex("three scans, three classes, an empty segment")
    assert set(map(tuple, r["table"][:, :2].tolist())) == {(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)}
    kept, dropped = ex("noise group kept"), ex("noise group dropped")
    assert kept["table"][:, 2].tolist() == [-1, 0, 1] and dropped["table"][:, 2].tolist() == [0, 1]
    assert kept["keep"].tolist() == [0, 1, 0] and np.array_equal(kept["labels"][0], dropped["labels"][0])
    r = ex("rejected rows")
    assert r["n_rejected"] == 5 and (r["labels"][0][[3, 11, 12, 40, 50, 60]] == -2).all() and r["labels"][0][51] == -1
    both = [ex(f"mixture {k}")["keep"] for k in range(20)]
    assert sum(int(k.sum()) for k in both) > 20 and sum(int((k == 0).sum()) for k in both) > 20


# ------------------------------------------------------------------------------------------------ parameters and arguments
def test_cluster_params_are_validated():
    from mopa_amd.objects import ClusterParams
    p = ClusterParams()
    assert (p.eps, p.min_samples, p.max_distance, p.include_noise) == (4.0, 5, 15.0, True)
    assert p.as_array().tolist() == [4.0, 5.0, 15.0, 1.0] and ClusterParams(include_noise=False).as_array()[3] == 0.0
    with pytest.raises(Exception):
        p.eps = 1.0                                         # frozen
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps="4"), dict(eps=True), dict(min_samples=0), dict(min_samples=2.5),
               dict(min_samples=True), dict(max_distance=float("inf")), dict(max_distance=None), dict(include_noise=1)):
        with pytest.raises(ValueError):
            ClusterParams(**kw)


def test_malformed_calls_are_named_before_any_device_is_touched():
    from mopa_amd import objects
    P, L, prm = np.zeros((10, 3), F32), np.zeros(10, np.int64), objects.ClusterParams()
    ok = dict(class_ids=[1], params=prm)
    bad_type = [
        dict(point_sets=P, label_sets=[L], **ok),                                  # an array where a list is expected
        dict(point_sets=[P], label_sets=L, **ok),
        dict(point_sets=[P.astype(np.float64)], label_sets=[L], **ok),
        dict(point_sets=[P.astype(np.float16)], label_sets=[L], **ok),
        dict(point_sets=[P], label_sets=[L.astype(np.int16)], **ok),
        dict(point_sets=[P], label_sets=[L.astype(F32)], **ok),
        dict(point_sets=[P, P], label_sets=[L, L.astype(np.int32)], **ok),
        dict(point_sets=[P.tolist()], label_sets=[L], **ok),
        dict(point_sets=[P], label_sets=[L], class_ids=[1], params=dict(eps=4)),
        dict(point_sets=[P], label_sets=[L], class_ids=[1.5], params=prm),
        dict(point_sets=[P], label_sets=[L], class_ids=7, params=prm),
        dict(point_sets=P, label_sets=L, counts="ab", **ok),
    ]
    for kw in bad_type:
        with pytest.raises(TypeError):
            objects.extract_instances_batch(**kw)
    bad_value = [
        dict(point_sets=[], label_sets=[], **ok),
        dict(point_sets=[P], label_sets=[L, L], **ok),
        dict(point_sets=[P[:, :2]], label_sets=[L], **ok),
        dict(point_sets=[P, np.zeros((4, 4), F32)], label_sets=[L, L[:4]], **ok),
        dict(point_sets=[P], label_sets=[L[:9]], **ok),
        dict(point_sets=[P], label_sets=[L[:, None]], **ok),
        dict(point_sets=[P], label_sets=[L], class_ids=[], params=prm),
        dict(point_sets=[P], label_sets=[L], class_ids=[1, 1], params=prm),
        dict(point_sets=[P], label_sets=[L], class_ids=list(range(33)), params=prm),
        dict(point_sets=[P], label_sets=[L], class_ids=[1 << 40], params=prm),
        dict(point_sets=P, label_sets=L, counts=[4, 5], **ok),
        dict(point_sets=P, label_sets=L, counts=[11, -1], **ok),
        dict(point_sets=np.zeros((0, 3), F32), label_sets=np.zeros(0, np.int64), counts=[0] * 40000, class_ids=[1, 2], params=prm),   # 80,000 segments
    ]
    for kw in bad_value:
        with pytest.raises(ValueError):
            objects.extract_instances_batch(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objects.extract_instances_batch([P], [L], [1], prm, device="cpu")
    with pytest.raises(TypeError):
        objects.extract_instances(P.tolist(), L, [1], prm)


def test_the_library_sizes_answer_on_the_host():
    from mopa_amd import _lib
    assert _lib.query("mopa_objects_rows_per_block") == 1024 and _lib.query("mopa_objects_max_classes") == 32
    assert _lib.query("mopa_objects_num_params") == 4
    assert _lib.query("mopa_objects_max_instances", 1000, 2, 3) == 1006
    small, large = _lib.query("mopa_objects_workspace_bytes", 1000, 1, 1, 1), _lib.query("mopa_objects_workspace_bytes", 100000, 99, 2, 3)
    assert 0 < small < large
    assert _lib.query("mopa_objects_workspace_bytes", 1000, 1, 1, 33) == 0 and _lib.query("mopa_objects_workspace_bytes", 1000, 5, 1, 1) == 0
    assert _lib.query("mopa_objects_launches") > 0         # no argument: the count follows neither the batch nor the classes


# ------------------------------------------------------------------------------------------------ the bank
def _instances(r, class_ids):
    """An Instances record on the host from a restatement result."""
    from mopa_amd.objects import Instances
    t = torch.from_numpy
    return Instances([t(x) for x in r["labels"]], t(r["table"]), t(r["offsets"]), t(r["mean_range"]), t(r["keep"]), t(r["points"]), r["n_rejected"],
                     tuple(class_ids))


@pytest.fixture(scope="module")
def results(cases):
    out = {}
    for name in ("mixture 8", "mixture 17", "five columns, uint8 labels, eps 1.5"):
        c = cases[name]
        prm = dict(ref.params_of(c), max_distance=60.0) if "five" in name else ref.params_of(c)    # 60 m: every class keeps some
        out[name] = (ref.extract(c["points"], c["labels"], c["class_ids"], **prm), c["class_ids"])
    return out


def test_the_bank_caps_in_the_references_order(results):
    from mopa_amd.objects import ObjectBank
    r, ids = results["mixture 8"]
    names = ["bicycle", "motorcycle", "pedestrian"]
    assert len(ids) == 3 and min(np.bincount(r["table"][r["keep"] == 1, 1], minlength=3)) >= 1
    for max_num in (1, 2, 100):
        bank = ObjectBank(names, ids, max_num)
        full = bank.add(_instances(r, ids))
        want = ref.capped(r, 3, max_num)
        assert full == all(len(w) == max_num for w in want)
        for name, w in zip(names, want):
            assert len(bank.objects[name]) == len(w) and all(np.array_equal(a, b) for a, b in zip(bank.objects[name], w)), (max_num, name)
    # two calls: the second one only fills what the first left open
    r2, _ = results["mixture 17"]
    bank = ObjectBank(names, ids, 3)
    bank.add(_instances(r, ids))
    first = {n: len(v) for n, v in bank.objects.items()}
    bank.add(_instances(r2, ids))
    w1, w2 = ref.capped(r, 3, 3), ref.capped(r2, 3, 3)
    for c, name in enumerate(names):
        want = (w1[c] + w2[c])[:3]
        assert first[name] == len(w1[c]) and len(bank.objects[name]) == len(want)
        assert all(np.array_equal(a, b) for a, b in zip(bank.objects[name], want))
    with pytest.raises(ValueError):
        ObjectBank(names, [1, 2, 3], 3).add(_instances(r, ids))        # other classes
    with pytest.raises(ValueError):
        ObjectBank(names[:2], ids, 3)
    with pytest.raises(ValueError):
        ObjectBank(names, ids, 0)


def test_the_bank_writes_and_reads_the_references_files(results, tmp_path):
    from mopa_amd.objects import ObjectBank
    r, ids = results["five columns, uint8 labels, eps 1.5"]
    names = ["bicycle", "motorcycle", "pedestrian"]
    bank = ObjectBank(names, ids, 1000)
    assert not bank.add(_instances(r, ids))
    want = ref.capped(r, 3, 1000)
    assert bank.dump(str(tmp_path)) == sum(len(w) for w in want) > 2
    for name, w in zip(names, want):
        assert sorted(os.listdir(tmp_path / name)) == ["{:05d}.bin".format(k + 1) for k in range(len(w))]
        for k, o in enumerate(w):
            assert (tmp_path / name / "{:05d}.bin".format(k + 1)).read_bytes() == np.ascontiguousarray(o, F32).tobytes()
    back = ObjectBank.load(str(tmp_path), names, cols=5)
    for name, w in zip(names, want):
        assert len(back.objects[name]) == len(w) and all(a.dtype == F32 and np.array_equal(a, b) for a, b in zip(back.objects[name], w))


def test_sample_draws_what_obj_sampling_draws(results, tmp_path):
    from mopa_amd.objects import ObjectBank
    r, ids = results["five columns, uint8 labels, eps 1.5"]
    names = ["bicycle", "motorcycle", "pedestrian"]
    bank = ObjectBank(names, ids, 1000)
    bank.add(_instances(r, ids))
    bank.dump(str(tmp_path))
    loaded = ObjectBank.load(str(tmp_path), names, cols=5)
    files = {n: sorted(str(p) for p in (tmp_path / n).glob("*.bin")) for n in names}
    order = [names[k % 3] for k in range(12)]
    np.random.seed(77)
    want = [ref.obj_sampling(files[n], 4 + names.index(n), 5) for n in order]
    after_want = np.random.rand()
    for b in (bank, loaded):
        np.random.seed(77)
        got = [b.sample(n, 4 + names.index(n)) for n in order]
        assert np.random.rand() == after_want                 # exactly the same draws were consumed
        for (pc, lab), (wpc, wlab) in zip(got, want):
            assert pc.dtype == F32 and np.array_equal(pc, wpc) and lab.dtype == np.float64 and np.array_equal(lab, wlab)
    bank.objects["bicycle"][0][0, 1] = np.nan
    with pytest.raises(AssertionError, match="Nan object points"):
        for _ in range(50):
            bank.sample("bicycle", 1)
