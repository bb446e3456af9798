"""tests/_supcon_reference.py, the yardstick of tests/test_gpu_supcon.py, against the reference's own ``SupConLoss`` and ``l2_norm`` in
float64 (tests/golden/g21_supcon.npz: tests/golden_gen/g21_supcon.py RAN them), and what of the Python layer needs no GPU.

Bounds: 4 x the worst distance the generator printed for the restatement with eps = 1e-5 against the reference's float64 autograd over
the seven cases -- loss 1.765e-16 (relative), gradient 1.522e-15 (of max |gradient|).  The fixture keeps the float64 gradients on at most
24 rows per side (its docstring says why); the comparison here runs on those rows, the recorded figures cover the full arrays.

The tests of the fixture, the restatement and its mutations are yardstick tests: they run no code of the package and hold the
yardstick itself; the argument checks, the size queries and the status constants are the package's."""
import os

import numpy as np
import pytest
import torch

import _supcon_reference as sref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_supcon.npz")
N_CASES = 7
LOSS_BOUND = 4 * 1.765e-16
GRAD_BOUND = 4 * 1.522e-15


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def case(golden, k):
    A = golden[f"c{k}_A"]
    shared = bool(golden["cases"][k][4])
    return golden[f"c{k}_la"], A, (A if shared else golden[f"c{k}_Q"]), golden[f"c{k}_lq"], shared


def errors(golden, k, **kw):
    la, A, Q, lq, shared = case(golden, k)
    r = sref.supcon(la, A, Q, lq, T=0.1, eps=1e-5, **kw)
    l64, gmax = float(golden[f"c{k}_loss64"]), float(golden[f"c{k}_gmax64"])
    ra = golden[f"c{k}_rows_a"]
    if shared:
        ge = np.abs((r["dA"] + r["dQ"])[ra] - golden[f"c{k}_dA64"]).max()
    else:
        ge = max(np.abs(r["dA"][ra] - golden[f"c{k}_dA64"]).max(), np.abs(r["dQ"][golden[f"c{k}_rows_q"]] - golden[f"c{k}_dQ64"]).max())
    return abs(r["loss"] - l64) / abs(l64), ge / gmax


def test_fixture_layout(golden):
    cases = golden["cases"]
    assert [tuple(int(v) for v in c[:4]) for c in cases] == [(5, 7, 3, 2), (65, 130, 16, 5), (33, 257, 128, 4), (129, 513, 64, 10),
                                                             (17, 40, 1, 2), (64, 64, 64, 3), (40, 50, 8, 3)]
    assert [int(c[4]) for c in cases] == [0, 0, 0, 0, 0, 1, 0] and [int(c[5]) for c in cases] == [1, 1, 1, 1, 1, 1, 6]
    assert "c5_Q" not in golden.files and golden["c0_A"].dtype == np.float32 and golden["c0_la"].dtype == np.int64
    for k in range(N_CASES):
        la, A, Q, lq, _ = case(golden, k)
        pos = (la[:, None] == lq[None, :]).sum(1)
        assert (pos > 0).all() and (pos < len(lq)).all()
        if k != 6:
            assert np.allclose(np.linalg.norm(A.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # the scaled case: most exp(S - m) fall below eps, and where a row's maximum is a positive, eps |N| carries D
    la, A, Q, lq, _ = case(golden, 6)
    r = sref.supcon(la, A, Q, lq, T=0.1)
    S = A.astype(np.float64) @ Q.astype(np.float64).T / 0.1
    assert (np.exp(S - r["m"][:, None]) < sref.EPS32).mean() > 0.5
    assert (sref.EPS32 * (la[:, None] != lq[None, :]).sum(1) / r["D"]).max() > 0.5
    assert os.path.getsize(GOLDEN) < (512 << 10)     # 425 KB: 345 KB of it the float32 inputs of the seven cases


@pytest.mark.parametrize("k", range(N_CASES))
def test_restatement_against_the_references_float64(golden, k):
    le, ge = errors(golden, k)
    print(f"case {k}: loss rel err {le:.3e} (bound {LOSS_BOUND:.3e}), grad err / max|grad| {ge:.3e} (bound {GRAD_BOUND:.3e}); recorded "
          f"{float(golden[f'c{k}_restatement_loss_err']):.3e} / {float(golden[f'c{k}_restatement_grad_err']):.3e}")
    assert le <= LOSS_BOUND and ge <= GRAD_BOUND


def test_bounds_are_the_recorded_ones(golden):
    assert max(float(golden[f"c{k}_restatement_loss_err"]) for k in range(N_CASES)) == pytest.approx(1.765e-16, rel=1e-3)
    assert max(float(golden[f"c{k}_restatement_grad_err"]) for k in range(N_CASES)) == pytest.approx(1.522e-15, rel=1e-3)
    # the reference's own float32 run, the budget of tests/test_gpu_supcon.py
    assert max(float(golden[f"c{k}_loss32_err"]) for k in range(N_CASES)) == pytest.approx(9.720e-08, rel=1e-3)
    assert max(float(golden[f"c{k}_grad32_err"]) for k in range(N_CASES)) == pytest.approx(5.900e-07, rel=1e-3)


@pytest.mark.parametrize("defect", ("all_in_denominator", "no_eps", "self_excluded"))
def test_mutations_leave_the_bound(golden, defect):
    moved = [k for k in range(N_CASES) if max(errors(golden, k, defect=defect)[0] / LOSS_BOUND, errors(golden, k, defect=defect)[1] / GRAD_BOUND) > 1]
    print(defect, "moves cases", moved)
    assert moved and (defect != "self_excluded" or moved == [5])


def test_shared_tensor_is_the_sum_of_both_sides(golden):
    la, A, Q, lq, shared = case(golden, 5)
    assert shared
    # the fixture's gradient of the ONE tensor is the sum of both sides (test_restatement_against_the_references_float64, case 5); here
    # central differences along a random direction, with eps = 0: the loss then does not depend on the detached m
    r = sref.supcon(la, A, A, lq, T=0.1, eps=0.0)
    rng = np.random.Generator(np.random.PCG64(1))
    d = rng.standard_normal(A.shape)
    h = 1e-6
    up = sref.supcon(la, A.astype(np.float64) + h * d, A.astype(np.float64) + h * d, lq, T=0.1, eps=0.0)["loss"]
    dn = sref.supcon(la, A.astype(np.float64) - h * d, A.astype(np.float64) - h * d, lq, T=0.1, eps=0.0)["loss"]
    assert (up - dn) / (2 * h) == pytest.approx(((r["dA"] + r["dQ"]) * d).sum(), rel=1e-5)
    assert np.abs(r["dA"]).max() > 0 and np.abs(r["dQ"]).max() > 0 and not np.allclose(r["dA"], r["dQ"])


def test_degenerate_rows():
    from mopa_amd.models import losses
    NO_POS, NO_NEG = losses.SUPCON_NO_POSITIVE, losses.SUPCON_NO_NEGATIVE      # the restatement's status word is the device's
    assert (NO_POS, NO_NEG, losses.SUPCON_NON_FINITE) == (1, 2, 4)
    rng = np.random.Generator(np.random.PCG64(2))
    A, Q = sref.unit_rows(rng, 6, 4), sref.unit_rows(rng, 9, 4)
    lq = np.asarray([0, 0, 0, 1, 1, 1, 2, 2, 2])
    la = np.asarray([0, 1, 2, 0, 1, 2])
    full = sref.supcon(la, A, Q, lq)
    assert full["status"] == 0 and np.isfinite(full["loss"]) and full["valid"].all()
    # one anchor without a positive
    la1 = la.copy()
    la1[2] = 7
    r = sref.supcon(la1, A, Q, lq)
    assert r["status"] == NO_POS and np.isnan(r["loss"]) and np.isnan(r["dA"]).all() and np.isnan(r["dQ"]).all()
    r = sref.supcon(la1, A, Q, lq, skip_invalid=True)
    keep = np.asarray([0, 1, 3, 4, 5])
    sub = sref.supcon(la1[keep], A[keep], Q, lq)
    assert r["status"] == NO_POS and r["loss"] == pytest.approx(sub["loss"], rel=1e-14)
    assert np.allclose(r["dA"][keep], sub["dA"], rtol=1e-13, atol=0) and not r["dA"][2].any() and np.allclose(r["dQ"], sub["dQ"], rtol=1e-12, atol=1e-18)
    # one anchor without a negative: a pool of a single class
    r = sref.supcon(np.asarray([0, 1]), A[:2], Q[:3], lq[:3])
    assert r["status"] == NO_POS | NO_NEG and np.isnan(r["loss"])        # anchor 0 has no negative, anchor 1 no positive
    r = sref.supcon(np.asarray([0, 1]), A[:2], Q[:3], lq[:3], skip_invalid=True)
    assert r["status"] == NO_POS | NO_NEG and r["loss"] == 0.0 and not r["dA"].any() and not r["dQ"].any()
    r = sref.supcon(np.asarray([0, 0]), A[:2], Q[:3], lq[:3])
    assert r["status"] == NO_NEG and np.isnan(r["loss"])


def test_l2_norm_restatement(golden):
    y, dx = sref.l2_norm(golden["l2_x"], golden["l2_g"])
    assert np.abs(y - golden["l2_y64"]).max() <= 1e-15
    assert (np.abs(dx - golden["l2_dx64"]).max(1) <= 4e-15 * np.abs(golden["l2_dx64"]).max(1)).all()
    x = golden["l2_x"].astype(np.float64)
    assert not y[0].any() and np.array_equal(dx[0], golden["l2_g"][0].astype(np.float64) / sref.L2_EPS)    # norm 0
    assert np.array_equal(y[1], x[1] / sref.L2_EPS) and np.array_equal(y[2], x[2] / sref.L2_EPS)           # below and exactly eps
    assert np.array_equal(dx[2], golden["l2_g"][2].astype(np.float64) / sref.L2_EPS)
    assert np.allclose(np.linalg.norm(y[3:], axis=1), 1.0, atol=1e-15)


def test_python_argument_checks_without_the_library(monkeypatch):
    from mopa_amd import _lib
    from mopa_amd.common.utils import loss as uloss
    from mopa_amd.models import losses
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(_lib, "query", lambda name, *a: calls.append(name))
    monkeypatch.setattr(uloss, "call", lambda name, *a: calls.append(name))
    z = torch.zeros
    y = lambda n: torch.zeros(n, dtype=torch.int64)     # noqa: E731
    for a, q, la, lq in ((z(4, 0), z(5, 0), y(4), y(5)), (z(4, 129), z(5, 129), y(4), y(5)), (z(4, 8), z(5, 9), y(4), y(5)),
                         (z(4, 8), z(5, 8), y(3), y(5)), (z(4, 8), z(5, 8), y(4), y(6)), (z(0, 8), z(5, 8), y(0), y(5)),
                         (z(4, 8), z(0, 8), y(4), y(0)), (z(4, 8, 1), z(5, 8), y(4), y(5))):
        with pytest.raises(ValueError):
            losses.supcon_loss(la, a, q, lq)
    for T in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            losses.SupConLoss(temperature=T)(y(4), z(4, 8), z(5, 8), y(5))
    with pytest.raises(TypeError, match="labels"):
        losses.supcon_loss(z(4), z(4, 8), z(5, 8), y(5))
    with pytest.raises(TypeError, match="features"):
        losses.supcon_loss(y(4), y(32).reshape(4, 8), z(5, 8), y(5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.SupConLoss()(y(4), z(4, 8), z(5, 8), y(5), iteration=3)
    with pytest.raises(ValueError):
        uloss.l2_norm(z(4, 129))
    with pytest.raises(ValueError):
        uloss.l2_norm(z(4))
    with pytest.raises(TypeError):
        uloss.l2_norm(y(8).reshape(2, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uloss.l2_norm(z(4, 8))
    assert calls == []
    m = losses.SupConLoss()
    assert m.temperature == 0.1 and m.skip_invalid is False


def test_workspace_and_chunks_are_functions_of_the_shape():
    from mopa_amd import _lib
    lib = _lib.load()
    assert 0 < lib.mopa_supcon_workspace_bytes(65536, 1 << 20, 64) <= 64 * (65536 + (1 << 20)) * 64 * 4
    assert lib.mopa_supcon_workspace_bytes(100, 100, 0) == 0 and lib.mopa_supcon_workspace_bytes(100, 100, 129) == 0
    assert lib.mopa_supcon_workspace_bytes(0, 100, 16) == 0 and lib.mopa_supcon_workspace_bytes(100, 0, 16) == 0
    assert lib.mopa_supcon_state_bytes(0) == 0 and lib.mopa_supcon_state_bytes(1000) == 16 + 12 * 1000
    # nothing grows like Na x Nq: doubling the pool at a large anchor count leaves the forward's partials where they were
    assert lib.mopa_supcon_workspace_bytes(65536, 1 << 21, 64) == lib.mopa_supcon_workspace_bytes(65536, 1 << 20, 64)
    for Na, Nq in ((1, 1), (65, 193), (4096, 65536), (1024, 8192), (1500, 10001), (10 ** 6, 10 ** 6)):
        ta, tq = -(-Na // lib.mopa_supcon_tile_rows(0)), -(-Nq // lib.mopa_supcon_tile_rows(1))
        want = min(64, tq, max(1, 1024 // ta))
        chunks = -(-tq // -(-tq // want))
        assert lib.mopa_supcon_pool_chunks(Na, Nq) == chunks
        assert lib.mopa_supcon_workspace_bytes(Na, Nq, 1) >= 28 * chunks * Na
    assert lib.mopa_supcon_pool_chunks(0, 5) == 0
    from mopa_amd.models import losses
    ta, tq = losses.supcon_tile_rows()
    assert (ta, tq) == (lib.mopa_supcon_tile_rows(0), lib.mopa_supcon_tile_rows(1)) and ta >= 32 and tq >= 32 and lib.mopa_supcon_tile_rows(2) == 0
