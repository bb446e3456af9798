"""Generate tests/golden/g19_logcoral.npz by RUNNING the reference's ``logcoral_loss`` (mopa/models/losses.py:47-93), loaded by path
from the checkout; its import of ``mopa.models.xmuda_arch`` is answered by a stub module, as in g12_minent.py.

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixture is what travels).
Usage, from the repo root:  python tests/golden_gen/g19_logcoral.py PATH_TO_MOPA_CHECKOUT

Per case ``k`` the .npz holds ``c<k>_src`` / ``c<k>_trg`` (float32 inputs: Gaussian rows times a random mixing matrix, plus the
case's column offset in column standard deviations; per case the first seeded draw whose covariances have condition numbers of at
most 1e7: tests/_coral_reference.py::conditioned_pair), ``c<k>_loss64`` and ``c<k>_dsrc64`` / ``c<k>_dtrg64`` (the reference's value and
autograd gradients on the inputs cast to float64) and, as scalars only, ``c<k>_loss32_err`` (|loss32 - loss64| / |loss64|) and
``c<k>_grad32_err`` (max |grad32 - grad64| / max |grad64| over both inputs) of the reference's own float32 run, plus ``c<k>_cond``
(the larger condition number of the two covariances) and ``c<k>_restatement_err`` (tests/_coral_reference.py against the float64
gradients, same measure).  ``cases`` holds (Ns, Nt, F, offset, ndim) rows.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _coral_reference as cref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g19_logcoral.npz")
# (Ns, Nt, F, column offset in standard deviations, shape of x_src or None, shape of x_trg or None)
CASES = ((17, 23, 16, 0, None, None), (40, 33, 5, 0, None, None), (65, 130, 64, 0, None, None), (257, 300, 64, 5, None, None),
         (300, 257, 16, 50, None, None), (64, 96, 16, 0, (4, 16, 16), (6, 16, 16)))


def _load(ref):
    stub = types.ModuleType("mopa.models.xmuda_arch")
    stub.batch_segment = lambda *a, **k: None
    for name in ("mopa", "mopa.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["mopa.models.xmuda_arch"] = stub
    spec = importlib.util.spec_from_file_location("ref_losses", os.path.join(ref, "mopa", "models", "losses.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.logcoral_loss


def inputs(k):
    Ns, Nt, F, off, shs, sht = CASES[k]
    return cref.conditioned_pair(19000 + 100 * k, Ns, Nt, F, off, shs, sht)


def main():
    logcoral_loss = _load(sys.argv[1])
    save = {"cases": np.asarray([(c[0], c[1], c[2], c[3], len(c[4]) if c[4] else 2) for c in CASES], np.int64)}
    for k in range(len(CASES)):
        xs, xt = inputs(k)
        save[f"c{k}_src"], save[f"c{k}_trg"] = xs, xt
        got = {}
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            a = torch.from_numpy(xs).to(dt).requires_grad_(True)
            b = torch.from_numpy(xt).to(dt).requires_grad_(True)
            loss = logcoral_loss(a, b)
            ga, gb = torch.autograd.grad(loss, (a, b))
            got[tag] = (float(loss.detach().double()), ga.double().numpy(), gb.double().numpy())
        l64, ga64, gb64 = got["64"]
        assert np.isfinite(l64) and np.isfinite(ga64).all() and np.isfinite(gb64).all()
        gmax = max(np.abs(ga64).max(), np.abs(gb64).max())
        save[f"c{k}_loss64"], save[f"c{k}_dsrc64"], save[f"c{k}_dtrg64"] = np.float64(l64), ga64, gb64
        save[f"c{k}_loss32_err"] = np.float64(abs(got["32"][0] - l64) / abs(l64))
        save[f"c{k}_grad32_err"] = np.float64(max(np.abs(got["32"][1] - ga64).max(), np.abs(got["32"][2] - gb64).max()) / gmax)
        r = cref.logcoral(xs, xt)
        save[f"c{k}_cond"] = np.float64(r["cond"])
        save[f"c{k}_restatement_err"] = np.float64(max(np.abs(r["d_src"] - ga64).max(), np.abs(r["d_trg"] - gb64).max()) / gmax)
        print(CASES[k][:4], "loss", l64, "cond %.2e" % r["cond"], "fp32 loss rel err %.2e" % save[f"c{k}_loss32_err"],
              "fp32 grad err / max|grad| %.2e" % save[f"c{k}_grad32_err"], "restatement: loss rel %.2e grad %.2e" %
              (abs(r["loss"] - l64) / abs(l64), save[f"c{k}_restatement_err"]))
    np.savez_compressed(OUT, **save)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
