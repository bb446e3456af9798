"""tests/_lovasz_reference.py, the yardstick of tests/test_gpu_lovasz.py, against the reference's own ``lovasz_softmax``
(tests/golden/g20_lovasz.npz: tests/golden_gen/g20_lovasz.py RAN it, in float32 -- it cannot run in float64).

The fixture records per case how far the float64 restatement is from the reference's float32 result; that distance is the reference's
own rounding (its weights come out of the float32 cancellation jaccard[1:] - jaccard[:-1]).  The bounds below are 4 x the worst
recorded figure; the factor covers the spread from case to case.  The mutation tests show that the bounds bite."""
import os

import numpy as np
import pytest

import _lovasz_reference as lref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_lovasz.npz")
N_CASES = 10
IGNORE = 255


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def bounds(golden):
    loss = max(float(golden[f"c{k}_loss_err"]) for k in range(N_CASES))
    grad = float(np.nanmax([float(golden[f"c{k}_grad_err"]) for k in range(N_CASES)]))
    return 4.0 * loss, 4.0 * grad


def restate(golden, k, **kw):
    """-> (loss, gradient in the layout of the fixture's probabilities) of the restatement on case k."""
    p, y = golden[f"c{k}_p"], golden[f"c{k}_y"]
    if p.ndim == 4:
        p2, y2, off = lref.from_nchw(p, y)
        r = lref.lovasz(p2, y2, ignore=IGNORE, offsets=off, **kw)
        return r["loss"], r["grad"].reshape(p.shape[0], p.shape[2], p.shape[3], p.shape[1]).transpose(0, 3, 1, 2)
    r = lref.lovasz(p, y, ignore=IGNORE, **kw)
    return r["loss"], r["grad"]


def errors(golden, k, **kw):
    loss, grad = restate(golden, k, **kw)
    ref_loss, ref_grad = float(golden[f"c{k}_loss"]), golden[f"c{k}_grad"].astype(np.float64)
    ties = bool(golden["cases"][k][4])
    return abs(loss - ref_loss) / abs(ref_loss), (np.nan if ties else np.abs(grad - ref_grad).max() / np.abs(ref_grad).max())


def test_fixture_layout(golden):
    cases = golden["cases"]
    assert cases.shape == (N_CASES, 6)
    assert {(int(c[0]), int(c[1])) for c in cases} >= {(17, 2), (64, 3), (257, 5), (1000, 10), (4097, 16)}
    assert {int(c[2]) for c in cases} >= {0, 200, 500, 900}
    assert sum(int(c[3]) for c in cases) == 1 and sum(int(c[4]) for c in cases) == 2
    assert golden["c7_p"].ndim == 4 and golden["c0_p"].dtype == np.float32 and golden["c0_grad"].dtype == np.float32
    y = golden["c5_y"]
    assert not (y == 3).any() and (y == 2).any()                      # a class absent
    assert set(np.unique(golden["c6_y"])) <= {1, IGNORE}              # all rows in a single class


@pytest.mark.parametrize("k", range(N_CASES))
def test_restatement_within_the_references_rounding(golden, bounds, k):
    """Bounds from this fixture: loss 4 x 7.263e-08 = 2.905e-07 (relative), gradient 4 x 1.594e-05 = 6.374e-05 (of max |grad|).
    Cases 8 and 9 hold exact ties: the loss only."""
    le, ge = errors(golden, k)
    print(f"case {k}: loss rel err {le:.3e} (bound {bounds[0]:.3e}), grad err / max|grad| {ge:.3e} (bound {bounds[1]:.3e})")
    assert le <= bounds[0]
    assert le == pytest.approx(float(golden[f"c{k}_loss_err"]), rel=1e-6, abs=1e-12)   # the figure the fixture recorded
    if not golden["cases"][k][4]:
        assert ge <= bounds[1]


def test_bounds_are_the_documented_ones(bounds):
    assert bounds[0] == pytest.approx(2.905e-07, rel=1e-3) and bounds[1] == pytest.approx(6.374e-05, rel=1e-3)


def test_one_valid_row():
    """V = 1: the single rank has w_0 = J_0 = 1 - (G - 1) / G = 1 for the row's class, the only one present: loss = e_0 = 1 - p."""
    p = np.asarray([[0.2, 0.5, 0.3], [0.1, 0.7, 0.2], [0.6, 0.3, 0.1]], np.float32)
    y = np.asarray([IGNORE, 2, IGNORE])
    r = lref.lovasz(p, y, ignore=IGNORE)
    e0 = float(np.float32(1.0) - p[1, 2])
    assert r["loss"] == e0
    want = np.zeros((3, 3))
    want[1, 2] = -1.0
    assert np.array_equal(r["grad"], want)
    one = lref.lovasz(p[1:2], y[1:2], ignore=IGNORE)
    assert one["loss"] == e0


def test_nothing_valid_or_nothing_selected():
    p = np.asarray([[0.2, 0.8], [0.6, 0.4]], np.float32)
    r = lref.lovasz(p, np.asarray([IGNORE, IGNORE]), ignore=IGNORE)
    assert r["loss"] == 0.0 and not r["grad"].any()
    r = lref.lovasz(p, np.asarray([7, 9]))                 # labels outside [0, C): foreground for no class, 'present' selects nothing
    assert r["loss"] == 0.0 and not r["grad"].any()
    r = lref.lovasz(p, np.asarray([7, 9]), classes="all")  # ... 'all': G = 0, J_k = 1, w = (1, 0): the largest p of each class
    assert r["loss"] == pytest.approx((0.6 + 0.8) / 2, rel=1e-7)
    r = lref.lovasz(p, np.asarray([0, 1]), classes=[])
    assert r["loss"] == 0.0 and not r["grad"].any()


def test_cross_tie_follows_the_stated_order():
    """Two rows, C = 2, p = 0.5: every error is 0.5, so the order is the row order (G = 1 for both classes).
    Ranks (fg, bg): I = (0, 0), U = (1, 2), J = (1, 1), w = (1, 0): L = 1/2, all the weight on the foreground row.
    Ranks (bg, fg): I = (1, 0), U = (2, 2), J = (1/2, 1), w = (1/2, 1/2): L = 1/2, the weight shared.
    The loss is 1/2 under either tie order (the extension is continuous); the gradient tells them apart."""
    p = np.full((2, 2), 0.5, np.float32)
    r = lref.lovasz(p, np.asarray([0, 1]))          # class 0: (fg, bg); class 1: (bg, fg)
    assert r["loss"] == 0.5
    assert np.array_equal(r["grad"], np.asarray([[-0.5, 0.25], [0.0, -0.25]]))
    r = lref.lovasz(p, np.asarray([1, 0]))          # class 0: (bg, fg); class 1: (fg, bg)
    assert r["loss"] == 0.5
    assert np.array_equal(r["grad"], np.asarray([[0.25, -0.5], [-0.25, 0.0]]))


def test_segments_and_logits_gradient(golden):
    p, y = golden["c2_p"], golden["c2_y"]
    off = [0, 100, 100, 257]
    r = lref.lovasz(p, y, ignore=IGNORE, offsets=off)
    parts = [lref.lovasz(p[a:b], y[a:b], ignore=IGNORE) if b > a else {"loss": 0.0} for a, b in zip(off[:-1], off[1:])]
    assert r["loss"] == pytest.approx(sum(q["loss"] for q in parts) / 3, rel=1e-15)
    # the chain rule through the softmax against the explicit Jacobian diag(p) - p p^T, row by row
    rng = np.random.Generator(np.random.PCG64(5))
    p32 = lref.softmax32(rng.standard_normal((6, 3)))
    yy = np.asarray([0, 1, 2, 1, 0, 2])
    dp = lref.lovasz(p32, yy)["grad"]
    dz = lref.logits_grad(p32, dp)
    for i in range(6):
        q = p32[i].astype(np.float64)
        assert np.allclose(dz[i], (np.diag(q) - np.outer(q, q)) @ dp[i], rtol=1e-13, atol=1e-16)
    assert np.abs(dz).max() > 0


@pytest.mark.parametrize("defect", ("ascending", "no_difference", "mean_over_C", "keep_ignored"))
def test_mutations_leave_the_bound(golden, bounds, defect):
    """Each one-defect variant of the restatement moves at least one fixture case beyond the bound that the restatement meets."""
    moved = []
    for k in range(N_CASES):
        le, ge = errors(golden, k, defect=defect)
        if le > bounds[0] or (not np.isnan(ge) and ge > bounds[1]):
            moved.append(k)
    print(defect, "moves cases", moved)
    assert moved
