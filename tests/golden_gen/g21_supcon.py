"""Generate tests/golden/g21_supcon.npz by RUNNING the reference's ``SupConLoss`` (mopa/models/losses.py:123-184) and ``l2_norm``
(mopa/common/utils/loss.py:230-238), loaded by path from the checkout with the stubs of g19_logcoral.py / g20_lovasz.py; both call
``.cuda()`` on a tensor they build, so ``torch.Tensor.cuda`` is patched to the identity for the run.

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixture is what travels).
Usage, from the repo root:  python tests/golden_gen/g21_supcon.py PATH_TO_MOPA_CHECKOUT

Per case ``k`` the reference runs twice, on float64 casts of the inputs (its 1e-5 is then the double) and on the float32 inputs (its own
value and gradients).  The .npz holds ``c<k>_A`` / ``c<k>_Q`` (float32; the shared-tensor case has no ``_Q``), ``c<k>_la`` / ``c<k>_lq``
(int64), ``c<k>_loss64``, ``c<k>_rows_a`` / ``c<k>_rows_q`` (the rows whose float64 gradients are kept: all of them up to 24, else
every ceil(N / 24)-th -- the full float64 gradients of the seven cases would be 690 KB) with ``c<k>_dA64`` / ``c<k>_dQ64`` on those rows,
``c<k>_gmax64`` (max |gradient| over BOTH full gradients) and, computed here over the FULL arrays, as scalars:
``c<k>_restatement_loss_err`` / ``c<k>_restatement_grad_err`` (tests/_supcon_reference.py with eps = 1e-5 against the float64 run:
|loss - loss64| / |loss64| and max |grad - grad64| / gmax64) and ``c<k>_loss32_err`` / ``c<k>_grad32_err`` (the float32 run against
the restatement with eps = float32(1e-5), same measures).  For the shared-tensor case the gradient is the one of the single tensor
(the sum of both sides) and lives in ``dA64``.  ``cases`` holds (Na, Nq, F, classes, shared, anchor scale) rows.  ``l2_*``: one
input with rows of norm 0, below, at and above eps, the reference's float64 output and gradient for the upstream ``l2_g``.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _supcon_reference as sref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g21_supcon.npz")
# (Na, Nq, F, classes, anchors and pool the same tensor, anchor scale)
CASES = ((5, 7, 3, 2, 0, 1), (65, 130, 16, 5, 0, 1), (33, 257, 128, 4, 0, 1), (129, 513, 64, 10, 0, 1), (17, 40, 1, 2, 0, 1),
         (64, 64, 64, 3, 1, 1), (40, 50, 8, 3, 0, 6))
KEEP_ROWS = 24


def _load(ref):
    stub = types.ModuleType("mopa.models.xmuda_arch")
    stub.batch_segment = lambda *a, **k: None
    for name in ("mopa", "mopa.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["mopa.models.xmuda_arch"] = stub
    try:
        import torchvision  # noqa: F401
    except ImportError:
        sys.modules["torchvision"] = types.ModuleType("torchvision")
    mods = []
    for name, rel in (("ref_losses", ("mopa", "models", "losses.py")), ("ref_loss", ("mopa", "common", "utils", "loss.py"))):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *rel))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    return mods[0].SupConLoss, mods[1].l2_norm


def inputs(k):
    Na, Nq, F, classes, shared, scale = CASES[k]
    rng = np.random.Generator(np.random.PCG64(21000 + 100 * k))
    Q = sref.unit_rows(rng, Nq, F)
    if shared:
        lq = rng.integers(0, classes, Nq).astype(np.int64)
        lq[:classes] = np.arange(classes)
        return Q, Q, lq, lq
    A = (sref.unit_rows(rng, Na, F) * np.float32(scale)).astype(np.float32)
    la, lq = sref.labels_with_both(rng, Na, Nq, classes)
    return A, Q, la, lq


def kept(n):
    return np.arange(0, n, -(-n // KEEP_ROWS) if n > KEEP_ROWS else 1)


def run_reference(crit, A, Q, la, lq, dt, shared):
    a = torch.from_numpy(A).to(dt).requires_grad_(True)
    q = a if shared else torch.from_numpy(Q).to(dt).requires_grad_(True)
    loss = crit(torch.from_numpy(la), a, q, torch.from_numpy(lq))
    grads = torch.autograd.grad(loss, (a,) if shared else (a, q))
    return float(loss.detach().double()), [t.double().numpy() for t in grads]


def main():
    SupConLoss, l2_norm = _load(sys.argv[1])
    torch.Tensor.cuda = lambda self, *a, **k: self
    crit = SupConLoss(temperature=0.1)
    save = {"cases": np.asarray(CASES, np.int64)}
    for k, (Na, Nq, F, classes, shared, scale) in enumerate(CASES):
        A, Q, la, lq = inputs(k)
        pos = (la[:, None] == lq[None, :]).sum(1)
        assert (pos > 0).all() and (pos < Nq).all(), "an anchor without a positive or without a negative"
        l64, g64 = run_reference(crit, A, Q, la, lq, torch.float64, shared)
        l32, g32 = run_reference(crit, A, Q, la, lq, torch.float32, shared)
        assert np.isfinite(l64) and all(np.isfinite(t).all() for t in g64) and np.isfinite(l32) and all(np.isfinite(t).all() for t in g32)
        r64 = sref.supcon(la, A, Q, lq, T=0.1, eps=1e-5)
        r32 = sref.supcon(la, A, Q, lq, T=0.1, eps=sref.EPS32)
        both = (lambda r: [r["dA"] + r["dQ"]]) if shared else (lambda r: [r["dA"], r["dQ"]])
        gmax = max(np.abs(t).max() for t in g64)
        save[f"c{k}_A"], save[f"c{k}_la"], save[f"c{k}_lq"] = A, la, lq
        if not shared:
            save[f"c{k}_Q"] = Q
        save[f"c{k}_loss64"], save[f"c{k}_gmax64"] = np.float64(l64), np.float64(gmax)
        save[f"c{k}_rows_a"] = kept(Na)
        save[f"c{k}_dA64"] = g64[0][kept(Na)]
        if not shared:
            save[f"c{k}_rows_q"] = kept(Nq)
            save[f"c{k}_dQ64"] = g64[1][kept(Nq)]
        e = {"restatement_loss_err": abs(r64["loss"] - l64) / abs(l64),
             "restatement_grad_err": max(np.abs(x - y).max() for x, y in zip(both(r64), g64)) / gmax,
             "loss32_err": abs(l32 - r32["loss"]) / abs(r32["loss"]),
             "grad32_err": max(np.abs(x - y).max() for x, y in zip(both(r32), g32)) / gmax}
        for name, v in e.items():
            save[f"c{k}_{name}"] = np.float64(v)
        print(CASES[k], "loss64 %.15g" % l64, " ".join(f"{n} {v:.3e}" for n, v in e.items()))
    # l2_norm: rows of norm 0, below eps, exactly eps, and ordinary ones
    rng = np.random.Generator(np.random.PCG64(21900))
    x = rng.standard_normal((8, 5)).astype(np.float32)
    x[0] = 0
    x[1] = np.asarray([3e-9, 0, 0, -4e-9, 0], np.float32)
    x[2] = np.asarray([0, sref.L2_EPS, 0, 0, 0], np.float32)
    x[3] *= np.float32(1e-6)
    g = rng.standard_normal((8, 5)).astype(np.float32)
    t = torch.from_numpy(x).double().requires_grad_(True)
    y = l2_norm(t)
    dx, = torch.autograd.grad(y, t, torch.from_numpy(g).double())
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    ry, rdx = sref.l2_norm(x, g)
    save["l2_x"], save["l2_g"], save["l2_y64"], save["l2_dx64"] = x, g, y.detach().numpy(), dx.numpy()
    print("l2_norm restatement: y err %.3e, dx err / max|dx| per row %.3e" %
          (np.abs(ry - save["l2_y64"]).max(), (np.abs(rdx - save["l2_dx64"]).max(1) / np.abs(save["l2_dx64"]).max(1)).max()))
    np.savez_compressed(OUT, **save)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
