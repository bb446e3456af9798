"""mopa_amd.models.losses.supcon_loss / SupConLoss and mopa_amd.common.utils.loss.l2_norm on the device (csrc/supcon.hip) against the
numpy float64 restatement tests/_supcon_reference.py on the same float32 inputs (T = float32(0.1) widened, eps = float32(1e-5) widened);
tests/test_supcon_host.py holds the restatement to the reference's own float64 autograd (tests/golden/g21_supcon.npz).

Bounds (u = 2^-24; computed per comparison by ``_supcon_reference.supcon(..., bounds=True)`` from the inputs, never from what the device
returns).  Model: every float32 rounding is an independent error, uniform in +-u |rounded value| (variance u^2 v^2 / 3); a sum of such
errors is held to six standard deviations.  expf's documented 1 ulp (2 u relative) is taken as one more such error of the pair's exponent.

  S_ij      the device forms S_ij as the fmaf chain over k = 0 .. F - 1 of v_mfma_f32_32x32x2_f32 from 0, then one division by T: every step
            rounds its partial sum s_k once, the division S_ij once: var(dS_ij) = (u^2 / 3) (sum_k s_k^2 / T^2 + S_ij^2), from the float64
            partial sums.  (The worst case of the same chain is the textbook gamma_F sum_k |a_ik q_jk| / T; at F = 64 it is thirty times
            the six-sigma figure and no wrong tile would ever reach it.)  A negative pair's exponent S_ij - m_i is rounded once more:
            and expf is applied: + (u^2 / 3) ((S_ij - m_i)^2 + 4).  m_i itself is the exact maximum of the device's own S.
  loss      mlpp_i is 2-Lipschitz in max_j |dS_ij|; to first order its error is sum_j c_ij dS_ij with c_ij = [P] / n_i - [N] exp(S_ij - m_i) /
            D_i, so var = sum_j c_ij^2 var(dS_ij).  The forward's float32 sums: E takes at most L - 1 = ceil(Nq / 64) - 1 additions and as
            many rescales per lane, five butterfly steps and one merge (relative variance (u^2 / 3) (2 L + 6), weighted by (E_i / D_i)^2 in
            log D_i); sum_P S is float32 only inside a lane (n_i terms in sums of at most L, (u^2 / 3) L^2 max_P |S|^2 / n_i after the division
            by n_i; nothing for L = 1) and float64 from the butterfly on.  The rows' errors are independent:
            loss bound = 6 sqrt(sum_i var_i) / divisor + 1e-13 (float64 sums).
  gradient  dA_if = c sum_j W_ij q_jf, c = -g / (divisor T).  The pair's own dS_ij: six sigma of sum_j (W_ij q_jf)^2 var(dS_ij).  Common to a
            row's negatives: the error of log D_i (six sigma as above).  Per term 4 u for expf, the product with 1 / D_i, 1 / n_i and
            the final store.  The second product is a float32 chain over the pool (flushed every 1,024 terms, splits added in float64):
            at most Nq + 64 roundings of partial sums no larger than sum_j |W_ij q_jf|, 6 sqrt((Nq + 64) / 3) u of it.  dQ alike, with the
            sums over the anchors.
What the model does not cover: errors that are NOT independent.  Where many pairs share one rounding the errors add up linearly and the
six-sigma figure is no longer a bound with that probability -- at F = 1 with unit-norm rows every S is +-fl(1 / T), one rounding shared by
all pairs, and the loss fills 0.86 of its bound (profiles/r38_supcon.md); inputs with many identical rows would do the same.  A
systematic error of that size in the kernel (a biased exp, a wrong rounding mode) could hide below the loss bound of a case whose
independent errors average out (four cases fill less than 0.01 of the loss bound); the per-element gradient bounds, which do not
average, are what catches a wrong tile or weight there (they fill 0.006 - 0.17).  The test cases use distinct random rows for that reason.
The float32 loss must be exactly the rounding of ``.loss64``.  Each test prints its worst err / bound (profiles/r38_supcon.md)."""
import os

import numpy as np
import pytest
import torch

import _supcon_reference as sref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_supcon.npz")
N_CASES = 7
T32 = float(np.float32(0.1))
# the reference's own float32 run against its float64 run, worst over the fixture (tests/test_supcon_host.py asserts these figures)
REF32_LOSS, REF32_GRAD = 9.720e-08, 5.900e-07
WIDTHS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128)


def _mod():
    from mopa_amd.models import losses
    return losses


def tiles():
    """(anchor rows, pool rows) per tile, as the library was compiled: the edge tests sit on these, whatever they are."""
    return _mod().supcon_tile_rows()


def edge(tile, mult, add):
    return mult * tile + add


EDGES = ((0, 1), (0, 2), (1, -1), (1, 0), (1, 1), (2, 1))      # (mult, add): 1, 2, T - 1, T, T + 1, 2 T + 1 rows for a tile of T


def test_tile_constants():
    from mopa_amd import _lib
    lib = _lib.load()
    assert tiles() == (lib.mopa_supcon_tile_rows(0), lib.mopa_supcon_tile_rows(1)) and min(tiles()) >= 32


def rand_case(seed, Na, Nq, F, classes=3, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    A = (sref.unit_rows(rng, Na, F) * np.float32(scale)).astype(np.float32)
    Q = (sref.unit_rows(rng, Nq, F) * np.float32(scale)).astype(np.float32)
    la, lq = sref.labels_with_both(rng, Na, Nq, classes)
    return la, A, Q, lq


def run(la, A, Q, lq, g=None, grad=(True, True), **kw):
    """-> (loss tensor, dA, dQ as float64 numpy or None)."""
    a = torch.from_numpy(A).cuda().requires_grad_(grad[0])
    q = torch.from_numpy(Q).cuda().requires_grad_(grad[1])
    loss = _mod().supcon_loss(torch.from_numpy(np.asarray(la)).cuda(), a, q, torch.from_numpy(np.asarray(lq)).cuda(), **kw)
    if loss.requires_grad:
        (loss if g is None else g * loss).backward()
    out = [None if t.grad is None else t.grad.cpu().numpy().astype(np.float64) for t in (a, q)]
    return loss, out[0], out[1]


def ratio(err, bound):
    return float((err / bound).max())


def check(got, ref, tag, status=0):
    loss, dA, dQ = got
    assert loss.dtype == torch.float32 and loss.dim() == 0
    l64 = float(loss.loss64)
    r = [abs(l64 - ref["loss"]) / ref["loss_bound"], ratio(np.abs(dA - ref["dA"]), ref["dA_bound"]), ratio(np.abs(dQ - ref["dQ"]), ref["dQ_bound"])]
    print(f"{tag}: loss64 {l64:.17g} ref {ref['loss']:.17g}; worst err / bound: loss {r[0]:.3f} dA {r[1]:.3f} dQ {r[2]:.3f}; status "
          f"{int(loss.status)}")
    assert float(loss.detach()) == float(np.float32(l64))
    assert int(loss.status) == status
    assert r[0] <= 1 and r[1] <= 1 and r[2] <= 1
    return r


def reference(la, A, Q, lq, **kw):
    return sref.supcon(la, A, Q, lq, T=T32, bounds=True, **kw)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("k", range(N_CASES))
def test_fixture_cases(golden, k):
    """Against the restatement within the derived bounds, and against the reference's float64 result within 4 x the distance of the
    reference's own float32 run (no worse than the reference in float32)."""
    A, la, lq = golden[f"c{k}_A"], golden[f"c{k}_la"], golden[f"c{k}_lq"]
    shared = bool(golden["cases"][k][4])
    gmax, l64 = float(golden[f"c{k}_gmax64"]), float(golden[f"c{k}_loss64"])
    ra = golden[f"c{k}_rows_a"]
    if shared:
        t = torch.from_numpy(A).cuda().requires_grad_(True)
        y = torch.from_numpy(la).cuda()
        loss = _mod().SupConLoss()(y, t, t, y)
        loss.backward()
        ref = reference(la, A, A, lq)
        got = t.grad.cpu().numpy().astype(np.float64)
        want, bound = ref["dA"] + ref["dQ"], ref["dA_bound"] + ref["dQ_bound"] + sref.U * np.abs(ref["dA"] + ref["dQ"])
        rl, rg = abs(float(loss.loss64) - ref["loss"]) / ref["loss_bound"], ratio(np.abs(got - want), bound)
        print(f"fixture case {k} (shared): worst err / bound: loss {rl:.3f} grad {rg:.3f}")
        assert rl <= 1 and rg <= 1 and int(loss.status) == 0
        dist_g = np.abs(got[ra] - golden[f"c{k}_dA64"]).max() / gmax
    else:
        Q = golden[f"c{k}_Q"]
        loss, dA, dQ = run(la, A, Q, lq)
        check((loss, dA, dQ), reference(la, A, Q, lq), f"fixture case {k}")
        dist_g = max(np.abs(dA[ra] - golden[f"c{k}_dA64"]).max(), np.abs(dQ[golden[f"c{k}_rows_q"]] - golden[f"c{k}_dQ64"]).max()) / gmax
    dist_l = abs(float(loss.loss64) - l64) / abs(l64)
    print(f"    distance from the reference's float64: loss {dist_l:.3e} (allowed {4 * REF32_LOSS:.3e}), grad {dist_g:.3e} "
          f"(allowed {4 * REF32_GRAD:.3e})")
    assert dist_l <= 4 * REF32_LOSS and dist_g <= 4 * REF32_GRAD


@pytest.mark.parametrize("mult,add", EDGES)
def test_anchor_tile_edges(mult, add):
    TA, TQ = tiles()
    Na = edge(TA, mult, add)
    c = rand_case(100 + Na, Na, TQ + 1, 16)
    check(run(*c), reference(*c), f"Na {Na} x Nq {TQ + 1}")


@pytest.mark.parametrize("mult,add", EDGES[1:])
def test_pool_tile_edges(mult, add):
    TA, TQ = tiles()
    Nq = edge(TQ, mult, add)
    c = rand_case(200 + Nq, TA + 1, Nq, 16, classes=2)
    check(run(*c), reference(*c), f"Na {TA + 1} x Nq {Nq}")


def test_pool_of_one_row():
    """Nq = 1: every anchor lacks a negative or a positive."""
    TA, TQ = tiles()
    la, A, Q, lq = rand_case(201, TA + 1, 1, 16, classes=2)
    la[::2] = lq[0] + 1
    loss, dA, dQ = run(la, A, Q, lq)
    assert int(loss.status) == 3 and np.isnan(float(loss.loss64)) and np.isnan(float(loss)) and np.isnan(dA).all() and np.isnan(dQ).all()
    loss, dA, dQ = run(la, A, Q, lq, skip_invalid=True)
    assert int(loss.status) == 3 and float(loss.loss64) == 0.0 and float(loss) == 0.0 and not dA.any() and not dQ.any()


def test_pool_chunks():
    """A pool over at least three chunks that ends one row past a chunk boundary; the row maximum in the last chunk."""
    from mopa_amd import _lib
    TA, TQ = tiles()
    Na, Nq = TA + 1, 3 * TQ + 1
    assert _lib.load().mopa_supcon_pool_chunks(Na, Nq) == 4
    la, A, Q, lq = rand_case(300, Na, Nq, 16)
    check(run(la, A, Q, lq), reference(la, A, Q, lq), "four chunks")
    Q[-1] = 3.0 * A[0]                       # S = 30 for anchor 0 in the last chunk's single row, everything before it within +-10
    for lab in (la[0], la[0] + 1):           # as a positive, and as a negative
        lq[-1] = lab
        ref = reference(la, A, Q, lq)
        assert ref["m"][0] == pytest.approx(30.0, rel=1e-6)
        check(run(la, A, Q, lq), ref, "maximum in the last chunk")
    # more tiles than chunks: 70 pool tiles at two anchor tiles -> ceil(70 / 64) = 2 tiles per chunk, 35 chunks
    Nq = 69 * TQ + 1
    assert _lib.load().mopa_supcon_pool_chunks(Na, Nq) == 35
    c = rand_case(301, Na, Nq, 8, classes=4)
    check(run(*c), reference(*c), "35 chunks of two tiles")


@pytest.mark.parametrize("F", WIDTHS)
def test_widths(F):
    c = rand_case(400 + F, 70, 150, F, classes=4)
    check(run(*c), reference(*c), f"F {F}")


def _all_nan(got, bits):
    loss, dA, dQ = got
    assert int(loss.status) == bits and np.isnan(float(loss.loss64)) and np.isnan(float(loss)) and np.isnan(dA).all() and np.isnan(dQ).all()


def test_anchors_without_a_positive():
    """Two anchors (in different tiles) whose class the pool does not hold: bit 0; NaN everywhere by default; left out under
    skip_invalid, where the divisor is the number of valid rows and their gradient rows are exact zeros."""
    la, A, Q, lq = rand_case(500, 70, 150, 16, classes=3)
    la[7], la[69] = 9, -4
    ref = reference(la, A, Q, lq)
    assert ref["status"] == 1 and np.isnan(ref["loss"])
    _all_nan(run(la, A, Q, lq), 1)
    got = run(la, A, Q, lq, skip_invalid=True)
    ref = reference(la, A, Q, lq, skip_invalid=True)
    assert ref["valid"].sum() == 68
    check(got, ref, "two anchors without a positive, skip_invalid", status=1)
    assert not got[1][7].any() and not got[1][69].any()


@pytest.mark.parametrize("others", ("same_class", "other_class"))
def test_anchor_without_a_negative(others):
    """An anchor has no negative only when the pool holds its class alone; every other anchor then lacks a negative too (same class:
    bit 1 alone) or a positive (another class: bits 0 and 1).  All anchors are invalid either way: NaN by default, exactly 0 with zero
    gradients under skip_invalid."""
    la, A, Q, lq = rand_case(510, 70, 150, 16, classes=2)
    lq[:] = 5
    la[:] = 5 if others == "same_class" else 6
    la[33] = 5
    bits = 2 if others == "same_class" else 3
    assert sref.supcon(la, A, Q, lq, T=T32)["status"] == bits
    _all_nan(run(la, A, Q, lq), bits)
    loss, dA, dQ = run(la, A, Q, lq, skip_invalid=True)
    assert int(loss.status) == bits and float(loss.loss64) == 0.0 and float(loss) == 0.0 and not dA.any() and not dQ.any()


def test_large_logits():
    """S over +-300: exp(S - m) underflows for most pairs, the running maximum's rescale multiplies by exp of at most 0."""
    TQ = tiles()[1]
    la, A, Q, lq = rand_case(600, 70, 3 * TQ + 5, 16, classes=3, scale=float(np.sqrt(30.0)))
    ref = reference(la, A, Q, lq)
    S = A.astype(np.float64) @ Q.astype(np.float64).T / T32
    assert S.max() > 200 and S.min() < -200
    got = run(la, A, Q, lq)
    assert np.isfinite(float(got[0].loss64)) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    check(got, ref, "S over +-300")
    # rising maxima: pool rows sorted by their S against anchor 0, so that its running maximum is replaced again and again
    order = np.argsort(S[0])
    Q, lq = Q[order], lq[order]
    check(run(la, A, Q, lq), reference(la, A, Q, lq), "rising maximum")


@pytest.mark.parametrize("where", ("first_chunk", "last_chunk"))
def test_non_finite_logits_set_bit_2(where):
    """One pool feature is +inf: the S of its column are +-inf or NaN.  Status bit 2 must come through the lane butterfly, the merge of the
    column halves, the chunk partials and the finalize, from the first and from the last of four chunks; the values are whatever IEEE
    arithmetic gives and are not compared."""
    TA, TQ = tiles()
    la, A, Q, lq = rand_case(650, TA + 1, 3 * TQ + 1, 16)
    clean = run(la, A, Q, lq)
    assert int(clean[0].status) == 0
    Q[5 if where == "first_chunk" else -1, 3] = np.inf
    loss, dA, dQ = run(la, A, Q, lq)
    assert int(loss.status) & _mod().SUPCON_NON_FINITE and int(loss.status) & 3 == 0
    assert not np.isfinite(float(loss.loss64))
    # a finite but overflowing product sets it as well
    Q[Q == np.inf] = 3e38
    A2 = A.copy()
    A2[:, 3] = 10.0
    assert int(run(la, A2, Q, lq)[0].status) & 4


def test_autograd_plumbing():
    L = _mod()
    la, A, Q, lq = rand_case(700, 70, 150, 16)
    ref = reference(la, A, Q, lq)
    base = run(la, A, Q, lq)
    check(base, ref, "base")
    y = lambda v: torch.from_numpy(v).cuda()     # noqa: E731
    # one side only
    only_a = run(la, A, Q, lq, grad=(True, False))
    assert only_a[2] is None and np.array_equal(only_a[1], base[1])
    only_q = run(la, A, Q, lq, grad=(False, True))
    assert only_q[1] is None and np.array_equal(only_q[2], base[2])
    # neither: no backward node
    none = run(la, A, Q, lq, grad=(False, False))
    assert not none[0].requires_grad and torch.equal(none[0], base[0])
    # the same tensor twice: the sum of both sides
    t = y(A).requires_grad_(True)
    loss = L.supcon_loss(y(la), t, t, y(la))
    loss.backward()
    both = run(la, A, A, la)
    assert torch.equal(loss, both[0])
    assert np.array_equal(t.grad.cpu().numpy().astype(np.float64), (torch.from_numpy(both[1]).float() + torch.from_numpy(both[2]).float()).double().numpy())
    # float16 features are cast: the float32 call on the same values, gradients in float16
    ha, hq = torch.from_numpy(A).half(), torch.from_numpy(Q).half()
    ta, tq = ha.cuda().requires_grad_(True), hq.cuda().requires_grad_(True)
    loss = L.supcon_loss(y(la), ta, tq, y(lq))
    loss.backward()
    want = run(la, ha.float().numpy(), hq.float().numpy(), lq)
    assert torch.equal(loss, want[0]) and ta.grad.dtype == torch.float16 and tq.grad.dtype == torch.float16
    assert np.array_equal(ta.grad.float().cpu().numpy(), want[1].astype(np.float32).astype(np.float16).astype(np.float32))
    # a strided view, int32 labels of another shape
    wide = torch.zeros(A.shape[0], 2 * A.shape[1])
    wide[:, ::2] = torch.from_numpy(A)
    v = wide.cuda()[:, ::2].detach().requires_grad_(True)
    q = y(Q).requires_grad_(True)
    loss = L.supcon_loss(y(la.astype(np.int32)).reshape(-1, 1), v, q, y(lq.astype(np.int32)).reshape(1, -1))
    loss.backward()
    assert torch.equal(loss, base[0]) and np.array_equal(v.grad.cpu().numpy().astype(np.float64), base[1])
    assert np.array_equal(q.grad.cpu().numpy().astype(np.float64), base[2])
    # an upstream gradient of 0.37, read from the device
    g = torch.tensor(0.37, device="cuda")
    scaled = run(la, A, Q, lq, g=g)
    rg = reference(la, A, Q, lq, g=float(np.float32(0.37)))
    check(scaled, rg, "g = 0.37")
    # the module form, the temperature and iteration arguments
    m = L.SupConLoss(temperature=0.5)
    a = y(A).requires_grad_(True)
    loss = m(y(la), a, y(Q), y(lq), iteration=12)
    r5 = sref.supcon(la, A, Q, lq, T=0.5, bounds=True)
    assert abs(float(loss.loss64) - r5["loss"]) <= r5["loss_bound"]


def test_same_bits_twice():
    la, A, Q, lq = rand_case(800, 1500, 10001, 64, classes=10)
    first = run(la, A, Q, lq)
    second = run(la, A, Q, lq)
    assert np.isfinite(float(first[0].loss64)) and int(first[0].status) == 0
    assert float(first[0].loss64) == float(second[0].loss64) and torch.equal(first[0], second[0])
    assert np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])
    # a coarse look at the value (the bounds are exercised at the small shapes): the restatement without its bound arrays
    ref = sref.supcon(la, A, Q, lq, T=T32)
    assert abs(float(first[0].loss64) - ref["loss"]) <= 4 * REF32_LOSS * abs(ref["loss"])
    gmax = max(np.abs(ref["dA"]).max(), np.abs(ref["dQ"]).max())
    assert max(np.abs(first[1] - ref["dA"]).max(), np.abs(first[2] - ref["dQ"]).max()) <= 4 * REF32_GRAD * gmax


@pytest.mark.parametrize("F", WIDTHS)
def test_l2_norm(F):
    """y: the norm is the float64 sum's square root rounded once to float32 (u) and the quotient once (u): |dy| <= 2^-23 |y|.
    dx above eps: (g - y (y . g)) / norm from the float32 y (2 u each), a float64 dot and one rounding:
    |d dx| <= 2^-22 (|g| + 3 |y| sum_k |y_k g_k|) / norm; at or below eps: g / eps, one rounding."""
    from mopa_amd.common.utils.loss import l2_norm
    rng = np.random.Generator(np.random.PCG64(900 + F))
    x = rng.standard_normal((37, F)).astype(np.float32)
    x[0] = 0
    x[1] = 0
    x[1, 0] = 5e-9
    x[2] = 0
    x[2, F - 1] = np.float32(1e-8)
    x[3] *= np.float32(1e-5)
    x[4] *= np.float32(1e4)
    g = rng.standard_normal((37, F)).astype(np.float32)
    t = torch.from_numpy(x).cuda().requires_grad_(True)
    y = l2_norm(t)
    y.backward(torch.from_numpy(g).cuda())
    ry, rdx = sref.l2_norm(x, g)
    gy, gdx = y.detach().cpu().numpy().astype(np.float64), t.grad.cpu().numpy().astype(np.float64)
    norm = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    above = norm > sref.L2_EPS
    assert list(above[:5]) == [False, False, False, True, True]
    by = 2.0 ** -23 * np.abs(ry) + 1e-44
    bdx = np.where(above[:, None], 2.0 ** -22 * (np.abs(g) + 3 * np.abs(ry) * np.abs(ry * g).sum(1, keepdims=True)) / np.maximum(norm, 1e-300)[:, None],
                   2.0 ** -24 * np.abs(rdx)) + 1e-44
    print(f"l2_norm F {F}: worst err / bound: y {ratio(np.abs(gy - ry), by):.3f} dx {ratio(np.abs(gdx - rdx), bdx):.3f}")
    assert (np.abs(gy - ry) <= by).all() and (np.abs(gdx - rdx) <= bdx).all()
    assert y.dtype == torch.float32 and not gy[0].any() and np.array_equal(gdx[0], (g[0] / np.float32(1e-8)).astype(np.float64))
    h = torch.from_numpy(x).half().cuda().requires_grad_(True)
    l2_norm(h).sum().backward()
    assert h.grad.dtype == torch.float16


def test_bad_arguments(monkeypatch):
    from mopa_amd import _lib
    from mopa_amd.common.utils import loss as uloss
    L = _mod()
    calls = []
    real_call, real_query = _lib.call, _lib.query
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(_lib, "query", lambda name, *a: (calls.append(name), real_query(name, *a))[1])
    monkeypatch.setattr(uloss, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    z = lambda *s: torch.zeros(*s, device="cuda")                    # noqa: E731
    y = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")  # noqa: E731
    for a, q, la, lq in ((z(4, 0), z(5, 0), y(4), y(5)), (z(4, 129), z(5, 129), y(4), y(5)), (z(4, 8), z(5, 9), y(4), y(5)),
                         (z(4, 8), z(5, 8), y(3), y(5)), (z(4, 8), z(5, 8), y(4), y(6)), (z(0, 8), z(5, 8), y(0), y(5)),
                         (z(4, 8), z(0, 8), y(4), y(0))):
        with pytest.raises(ValueError):
            L.supcon_loss(la, a, q, lq)
    with pytest.raises(ValueError, match="temperature"):
        L.supcon_loss(y(4), z(4, 8), z(5, 8), y(5), temperature=0.0)
    with pytest.raises(TypeError, match="labels"):
        L.supcon_loss(z(4), z(4, 8), z(5, 8), y(5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.supcon_loss(y(4).cpu(), torch.zeros(4, 8), torch.zeros(5, 8), y(5).cpu())
    with pytest.raises(ValueError):
        uloss.l2_norm(z(4, 129))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uloss.l2_norm(torch.zeros(4, 8))
    assert calls == []
    # the C entry points refuse the same shapes themselves, before any launch
    lib = _lib.load()
    buf, lab = z(1 << 16), y(1 << 10)
    p, l = buf.data_ptr(), lab.data_ptr()

    def fwd(Na, Nq, F, T=0.1, skip=0):
        return lib.mopa_supcon_fwd(l, p, Na, p, l, Nq, F, T, skip, p, p, p, p, 1 << 18, None)

    def bwd(Na, Nq, F, T=0.1, side=0):
        return lib.mopa_supcon_bwd(l, p, Na, p, l, Nq, F, T, side, p, p, p, p, 1 << 18, None)

    for f in (fwd, bwd):
        assert f(4, 5, 0) == -1 and f(4, 5, 129) == -1 and f(0, 5, 8) == -1 and f(4, 0, 8) == -1 and f(4, 5, 8, T=0.0) == -1
        assert f(4, 5, 8, T=-1.0) == -1 and f(4, 5, 8, T=float("nan")) == -1
    assert fwd(4, 5, 8, skip=2) == -1 and bwd(4, 5, 8, side=2) == -1
    assert lib.mopa_supcon_fwd(l, p, 4, p, l, 5, 8, 0.1, 0, p, p, p, p, 16, None) == -2      # workspace too small
    assert lib.mopa_l2norm_rows_fwd(p, 4, 0, p, p, None) == -1 and lib.mopa_l2norm_rows_fwd(p, 4, 129, p, p, None) == -1
    assert lib.mopa_l2norm_rows_fwd(p, 0, 8, p, p, None) == -1 and lib.mopa_l2norm_rows_bwd(p, p, p, 4, 129, p, None) == -1
    torch.cuda.synchronize()
