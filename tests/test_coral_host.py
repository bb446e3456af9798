"""logCORAL without a GPU: the numpy float64 restatement (tests/_coral_reference.py, the yardstick of tests/test_gpu_coral.py)
against the reference's own float64 autograd recorded in tests/golden/g19_logcoral.npz (tests/golden_gen/g19_logcoral.py RAN the
reference's function), the premise of computing in float64 (the reference's float32 gradient is off by more than 1e-4 of its largest
element on the (65, 130, 64) case), and the argument checks of mopa_amd.models.losses.logcoral_loss that need no device.

Bound of the restatement against the fixture: |loss - loss64| <= 1e-8 |loss64|, per gradient element
|err| <= 2^-23 |ref| + 1e-8 max|ref| -- the bound the device is held to; the generator measured 3.4e-11 at worst on these cases."""
import os

import numpy as np
import pytest
import torch

import _coral_reference as cref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_logcoral.npz")
CASES = ((17, 23, 16, 0, 2), (40, 33, 5, 0, 2), (65, 130, 64, 0, 2), (257, 300, 64, 5, 2), (300, 257, 16, 50, 2), (64, 96, 16, 0, 3))


def grad_bound(ref):
    return 2.0 ** -23 * np.abs(ref) + 1e-8 * np.abs(ref).max()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_holds_the_cases_the_issue_names(golden):
    assert [tuple(int(v) for v in row) for row in golden["cases"]] == list(CASES)
    assert golden["c5_src"].shape == (4, 16, 16) and golden["c5_trg"].shape == (6, 16, 16)     # pins factor = 1 / 3
    for k, (ns, nt, f, off, nd) in enumerate(CASES):
        assert golden[f"c{k}_src"].dtype == np.float32 and golden[f"c{k}_dsrc64"].dtype == np.float64
        assert golden[f"c{k}_dsrc64"].shape == golden[f"c{k}_src"].shape and golden[f"c{k}_dtrg64"].shape == golden[f"c{k}_trg"].shape
        assert float(golden[f"c{k}_cond"]) <= cref.COND_MAX
        if off:   # the columns really sit `off` standard deviations from zero
            x = golden[f"c{k}_src"].astype(np.float64)
            assert np.all(np.abs(x.mean(0) / x.std(0)) > 0.5 * off)
    assert os.path.getsize(GOLDEN) < 700_000


@pytest.mark.parametrize("k", range(len(CASES)))
def test_restatement_matches_the_reference_fp64(golden, k):
    r = cref.logcoral(golden[f"c{k}_src"], golden[f"c{k}_trg"])
    l64 = float(golden[f"c{k}_loss64"])
    print(CASES[k], "loss rel err", abs(r["loss"] - l64) / abs(l64))
    assert not r["guard"] and abs(r["loss"] - l64) <= 1e-8 * abs(l64)
    for key, ref in (("d_src", golden[f"c{k}_dsrc64"]), ("d_trg", golden[f"c{k}_dtrg64"])):
        err = np.abs(r[key] - ref)
        print("  ", key, "max err / max|ref|", err.max() / np.abs(ref).max())
        assert np.all(err <= grad_bound(ref))
    assert float(golden[f"c{k}_restatement_err"]) <= 1.3e-10     # the figure the 1e-8 term is 75 times of


def test_three_dimensional_case_uses_the_first_dimension(golden):
    """factor = 1 / (4 - 1) for both sides.  Because BOTH covariances carry the same factor, log(f C) = log(f) I + log(C) cancels it in
    L_src - L_trg: loss and gradient do not depend on it, only the guard does -- a (4, 16, 16) input whose largest covariance entry
    is 3e30 under 1 / 3 trips it, the same values as (64, 16) rows (factor 1 / 63) do not."""
    xs, xt = golden["c5_src"], golden["c5_trg"]
    flat = cref.logcoral(xs.reshape(-1, 16), xt.reshape(-1, 16))
    assert abs(flat["loss"] - float(golden["c5_loss64"])) <= 1e-12 * float(golden["c5_loss64"])
    assert np.allclose(flat["d_src"].reshape(4, 16, 16), golden["c5_dsrc64"], rtol=0, atol=1e-10 * np.abs(golden["c5_dsrc64"]).max())
    big_s, big_t = cref.guard_threshold_pair(xs, xt)
    assert cref.logcoral(big_s, big_t)["guard"] and not cref.logcoral(big_s.reshape(-1, 16), big_t.reshape(-1, 16))["guard"]


def test_reference_fp32_gradient_is_off(golden):
    """The premise of the float64 device path: the reference's own float32 run misses its float64 gradient by more than 1e-4 of the
    largest element at 64 features from 65 rows."""
    assert CASES[2] == (65, 130, 64, 0, 2)
    assert float(golden["c2_grad32_err"]) > 1e-4


def test_guard_and_limits_of_the_restatement():
    rng = np.random.Generator(np.random.PCG64(5))
    xs, xt = cref.mixed_gaussian(rng, 20, 4), cref.mixed_gaussian(rng, 20, 4)
    bad = xt.copy()
    bad[3, 1] = np.nan
    for t in (bad, xt * np.float32(1e20)):
        r = cref.logcoral(xs, t)
        assert r["guard"] and r["loss"] == 0.0 and not r["d_src"].any() and not r["d_trg"].any()
    # repeated eigenvalues: the limit 1 / lambda, finite
    K = cref.divided_differences(np.array([2.0, 2.0, 2.0 * (1 + 1e-12), 5.0]))
    assert np.isfinite(K).all() and np.allclose(K[:3, :3], 0.5, rtol=1e-11) and np.isclose(K[0, 3], np.log(2.5) / 3.0, rtol=1e-14)
    assert np.array_equal(K, K.T)


def test_argument_checks_without_a_device():
    from mopa_amd.models.losses import MAX_FEATURES, logcoral_loss
    assert MAX_FEATURES == 64
    z = torch.zeros
    with pytest.raises(ValueError, match="64"):
        logcoral_loss(z(8, 65), z(8, 65))
    with pytest.raises(ValueError, match="widths differ"):
        logcoral_loss(z(8, 16), z(8, 15))
    with pytest.raises(ValueError, match="two dimensions"):
        logcoral_loss(z(8), z(8))
    with pytest.raises(ZeroDivisionError):
        logcoral_loss(z(1, 8, 16), z(2, 8, 16))
    with pytest.raises(ValueError, match="fewer than two rows"):
        logcoral_loss(z(2, 16), z(1, 16))
    with pytest.raises(TypeError):
        logcoral_loss(z(8, 16, dtype=torch.int64), z(8, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        logcoral_loss(z(8, 16), z(8, 16))


def test_entry_points_refuse_bad_arguments():
    """Checked at the entry point before any launch: 1 <= F <= 64, row counts, pointers (no GPU needed: every call returns -1)."""
    from mopa_amd import _lib
    lib = _lib.load()
    assert _lib.query("mopa_logcoral_workspace_bytes", 0) == 0 and _lib.query("mopa_logcoral_workspace_bytes", 65) == 0
    assert _lib.query("mopa_logcoral_state_bytes", 65) == 0
    assert _lib.query("mopa_logcoral_state_bytes", 64) == 8 * (2 + 2 * 64 + 2 * 64 * 64)
    ws16, ws64 = _lib.query("mopa_logcoral_workspace_bytes", 16), _lib.query("mopa_logcoral_workspace_bytes", 64)
    assert 0 < ws16 < ws64 <= 32 << 20          # a fixed number of slabs: no dependence on the row count
    p = 4096                                    # a non-null, aligned address that is never dereferenced: every call below is refused
    good = dict(xs=p, ns=10, xt=p, nt=10, F=16, bs=10, loss=p, state=p, status=p, ws=p, wsb=ws16)

    def fwd(**kw):
        a = dict(good, **kw)
        return lib.mopa_logcoral_fwd(a["xs"], a["ns"], a["xt"], a["nt"], a["F"], a["bs"], a["loss"], a["state"], a["status"], a["ws"],
                                     a["wsb"], None)

    for kw in (dict(F=0), dict(F=65), dict(ns=1), dict(nt=1), dict(bs=1), dict(xs=None), dict(xt=None), dict(loss=None), dict(state=None),
               dict(status=None), dict(ws=None), dict(state=p + 4)):
        assert fwd(**kw) == -1, kw
    assert fwd(wsb=ws16 - 8) == -2
    for args in ((None, 10, 16, 0, p, p, p, p), (p, 1, 16, 0, p, p, p, p), (p, 10, 65, 0, p, p, p, p), (p, 10, 16, 2, p, p, p, p),
                 (p, 10, 16, 0, None, p, p, p), (p, 10, 16, 0, p, None, p, p), (p, 10, 16, 0, p, p, None, p), (p, 10, 16, 0, p, p, p, None)):
        assert lib.mopa_logcoral_bwd(*args, None) == -1, args
