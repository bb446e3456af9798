"""mopa_amd.models.losses.logcoral_loss on the device (csrc/coral.hip) against the reference's float64 autograd
(tests/golden/g19_logcoral.npz: tests/golden_gen/g19_logcoral.py RAN the reference's function) and, where the fixture has no case,
against the numpy float64 restatement tests/_coral_reference.py, which tests/test_coral_host.py holds to the same fixture.

Bound (every comparison below): |loss - loss64| <= 1e-8 |loss64| and per gradient element |err| <= 2^-23 |ref| + 1e-8 max|ref|.  The
first gradient term is the one float32 rounding of the stored gradient; the second is 75 times the worst agreement (1.3e-10) between
the restatement and the reference's float64 (this fixture's own worst is 3.4e-11, so the bound stands as stated).  The loss bound is
applied to ``.loss64``, the float64 value the kernel computed (a float32 cannot be within 1e-8 of anything); the returned float32
must be exactly its rounding.

Inputs outside the fixture are Gaussian rows times a random mixing matrix with covariance condition numbers of at most 1e7
(_coral_reference.conditioned_pair); rank-deficient inputs are not compared (the reference's own result there is rounding noise)."""
import os

import numpy as np
import pytest
import torch

import _coral_reference as cref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_logcoral.npz")
N_CASES = 6
# csrc/coral.hip walks 64-row tiles with at most 256 blocks per input: every block of a full grid loops at least twice over its rows
# from N = (2 * 256 - 1) * 64 + 1 = 32705 rows on.  The two row counts the big cases use lie above it (782 and 1094 tiles: three to
# five walks per block, ragged last tiles of 37 and 49 rows).
TWO_WALKS_N = (2 * 256 - 1) * 64 + 1
BIG = (70001, 50021)


def _loss_fn():
    from mopa_amd.models.losses import logcoral_loss
    return logcoral_loss


def run(xs, xt, scale=None, grad=(True, True)):
    """-> (loss tensor, d_src, d_trg) of the device call on numpy / torch inputs; gradients as float64 numpy (None without)."""
    a = (torch.from_numpy(xs) if isinstance(xs, np.ndarray) else xs).cuda().requires_grad_(grad[0])
    b = (torch.from_numpy(xt) if isinstance(xt, np.ndarray) else xt).cuda().requires_grad_(grad[1])
    loss = _loss_fn()(a, b)
    if any(grad):
        (loss if scale is None else scale * loss).backward()
    return loss, a.grad, b.grad


def check(loss, ga, gb, ref_loss, ref_a, ref_b, tag):
    assert loss.dtype == torch.float32 and loss.dim() == 0
    l64 = float(loss.loss64)
    print(tag, "loss rel err %.2e" % (abs(l64 - ref_loss) / abs(ref_loss)), "status", int(loss.status))
    assert abs(l64 - ref_loss) <= 1e-8 * abs(ref_loss)
    assert float(loss.detach()) == float(np.float32(l64))
    assert int(loss.status) == 0
    for name, g, ref in (("d_src", ga, ref_a), ("d_trg", gb, ref_b)):
        assert g.dtype == torch.float32 and tuple(g.shape) == ref.shape
        err = np.abs(g.cpu().numpy().astype(np.float64) - ref)
        bound = 2.0 ** -23 * np.abs(ref) + 1e-8 * np.abs(ref).max()
        print("   ", name, "max err / max|ref| %.2e" % (err.max() / np.abs(ref).max()), "worst err / bound %.3f" % (err / bound).max())
        assert np.all(err <= bound)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("k", range(N_CASES))
def test_parity_with_the_reference_fp64(golden, k):
    loss, ga, gb = run(golden[f"c{k}_src"], golden[f"c{k}_trg"])
    check(loss, ga, gb, float(golden[f"c{k}_loss64"]), golden[f"c{k}_dsrc64"], golden[f"c{k}_dtrg64"], f"case {k}")


@pytest.mark.parametrize("F", (64, 16))
def test_rows_beyond_one_block_walk(F):
    assert min(BIG) >= TWO_WALKS_N
    xs, xt = cref.conditioned_pair(700 + F, BIG[0], BIG[1], F, offset=2.0)
    r = cref.logcoral(xs, xt)
    loss, ga, gb = run(xs, xt)
    check(loss, ga, gb, r["loss"], r["d_src"], r["d_trg"], f"rows {BIG} F {F}")


@pytest.mark.parametrize("F", (1, 2, 3, 63, 64))
def test_small_and_padded_widths(F):
    """N = F + 1 rows on the source side, F + 2 on the target side: the fewest rows with a full-rank covariance; odd F is padded in the
    Jacobi stage, F < 4 and F = 63 leave part of a 4 x 4 patch empty."""
    xs, xt = cref.conditioned_pair(900 + F, F + 1, F + 2, F)
    r = cref.logcoral(xs, xt)
    loss, ga, gb = run(xs, xt)
    check(loss, ga, gb, r["loss"], r["d_src"], r["d_trg"], f"F {F} cond {r['cond']:.1e}")


def _hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


@pytest.mark.parametrize("F,scales", ((8, (1.0, 1.0)), (15, (1.0, 3.0)), (16, (0.5, 1.0))))
def test_repeated_eigenvalues_take_the_limit(F, scales):
    """Columns 1..F of a Hadamard matrix have zero mean and are orthogonal: cov is an exact multiple of the identity on both sides
    (32 and 64 rows: different multiples, so the gradient is not zero).  The reference's SVD backward gives 0/0 here; the device
    takes 1 / lambda."""
    xs = (scales[0] * _hadamard(32)[:, 1:F + 1]).astype(np.float32)
    xt = (scales[1] * _hadamard(64)[:, 1:F + 1]).astype(np.float32)
    r = cref.logcoral(xs, xt)
    assert r["loss"] > 0 and np.abs(r["d_src"]).max() > 0
    loss, ga, gb = run(xs, xt)
    assert torch.isfinite(ga).all() and torch.isfinite(gb).all()
    check(loss, ga, gb, r["loss"], r["d_src"], r["d_trg"], f"hadamard F {F}")


def test_guard(golden):
    xs, xt = golden["c0_src"], golden["c0_trg"]
    clean, _, _ = run(xs, xt)
    assert int(clean.status) == 0 and float(clean.detach()) > 0
    nan = xt.copy()
    nan[5, 3] = np.nan
    big_s, big_t = cref.guard_threshold_pair(golden["c5_src"], golden["c5_trg"])     # trips under 1 / 3, not under 1 / 63
    for a, b in ((xs, nan), (xs, xt * np.float32(1e20)), (xs * np.float32(1e20), xt), (big_s, big_t)):
        loss, ga, gb = run(a, b)
        assert int(loss.status) & 1
        assert float(loss.detach()) == 0.0 and float(loss.loss64) == 0.0
        assert ga.shape == a.shape and gb.shape == b.shape
        assert not ga.any() and not gb.any() and torch.isfinite(ga).all() and torch.isfinite(gb).all()
    # the same values flattened first: factor 1 / 63, below the threshold, the usual result (the common factor cancels in the loss)
    loss, ga, gb = run(big_s.reshape(-1, 16), big_t.reshape(-1, 16))
    want = cref.logcoral(big_s.reshape(-1, 16), big_t.reshape(-1, 16), grad=False)["loss"]
    assert int(loss.status) == 0 and abs(float(loss.loss64) - want) <= 1e-8 * want


def test_same_bits_on_every_run(golden):
    xs, xt = cref.conditioned_pair(764, BIG[0], BIG[1], 64, offset=2.0)
    first = run(xs, xt)
    second = run(xs, xt)
    assert float(first[0].loss64) == float(second[0].loss64) and torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])
    a = run(golden["c2_src"], golden["c2_trg"])
    b = run(golden["c2_src"], golden["c2_trg"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_autograd(golden, monkeypatch):
    from mopa_amd import _lib
    xs, xt = golden["c3_src"], golden["c3_trg"]
    full = run(xs, xt)
    half = run(xs, xt, scale=0.5)
    assert torch.equal(half[1], 0.5 * full[1]) and torch.equal(half[2], 0.5 * full[2])
    # an input without requires_grad: no launch for it, a None gradient
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a[3] if name == "mopa_logcoral_bwd" else None)), real(name, *a))[1])
    only_t = run(xs, xt, grad=(False, True))
    assert only_t[1] is None and torch.equal(only_t[2], full[2])
    assert [c for c in calls if c[0] == "mopa_logcoral_bwd"] == [("mopa_logcoral_bwd", 1)]
    calls.clear()
    only_s = run(xs, xt, grad=(True, False))
    assert only_s[2] is None and torch.equal(only_s[1], full[1])
    assert [c for c in calls if c[0] == "mopa_logcoral_bwd"] == [("mopa_logcoral_bwd", 0)]
    calls.clear()
    neither, _, _ = run(xs, xt, grad=(False, False))
    assert not neither.requires_grad and torch.equal(neither, full[0]) and [c[0] for c in calls] == ["mopa_logcoral_fwd"]
    monkeypatch.undo()
    # a non-contiguous float32 view of the same values
    wide = torch.zeros(xs.shape[0], 2 * xs.shape[1])
    wide[:, ::2] = torch.from_numpy(xs)
    wide = wide.cuda()
    view = wide[:, ::2].detach().requires_grad_(True)
    assert not view.is_contiguous()
    b = torch.from_numpy(xt).cuda().requires_grad_(True)
    loss = _loss_fn()(view, b)
    loss.backward()
    assert torch.equal(loss, full[0]) and torch.equal(view.grad, full[1]) and torch.equal(b.grad, full[2])
    # float16 inputs are cast: the same result as the float32 call on the same (half-representable) values
    h_s, h_t = torch.from_numpy(golden["c0_src"]).half(), torch.from_numpy(golden["c0_trg"]).half()
    ref = run(h_s.float(), h_t.float())
    got = run(h_s, h_t)
    assert torch.equal(got[0], ref[0]) and got[1].dtype == torch.float16
    assert torch.equal(got[1], ref[1].half()) and torch.equal(got[2], ref[2].half())
    # three-dimensional inputs get gradients of their own shape (the parity test covers the values)
    assert run(golden["c5_src"], golden["c5_trg"])[1].shape == (4, 16, 16)


def test_refusals():
    f = _loss_fn()
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    with pytest.raises(ValueError, match="64"):
        f(z(8, 65), z(8, 65))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(torch.zeros(8, 16), z(8, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(z(8, 16), torch.zeros(8, 16))
    with pytest.raises(ZeroDivisionError):
        f(z(1, 16), z(8, 16))
    with pytest.raises(ZeroDivisionError):
        f(z(1, 8, 16), z(2, 8, 16))
    with pytest.raises(ValueError, match="fewer than two rows"):
        f(z(8, 16), z(1, 16))
