"""Generate tests/golden/g20_lovasz.npz by RUNNING the reference's ``lovasz_softmax`` (mopa/common/utils/loss.py:122-199), loaded by path
from the checkout as g19_logcoral.py does; its top-level ``import torchvision`` is answered by an empty stub module when the package is
not installed.

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixture is what travels).
Usage, from the repo root:  python tests/golden_gen/g20_lovasz.py PATH_TO_MOPA_CHECKOUT

The reference cannot run in float64 (``lovasz_grad`` casts to float and ``torch.dot`` then refuses the mixed types), so the fixture holds
its float32 loss and float32 autograd gradient.  Per case ``k``: ``c<k>_p`` (float32 probabilities: the softmax of Gaussian logits
times 3; (P, C) or (B, C, H, W)), ``c<k>_y`` (int64 labels, 255 = ignored), ``c<k>_loss`` / ``c<k>_grad`` (the reference's), and as
scalars ``c<k>_loss_err`` = |restatement - reference| / |reference| and ``c<k>_grad_err`` = max |restatement - reference| / max
|reference| (tests/_lovasz_reference.py; NaN for the cases with exact ties, where the reference's order and with it its gradient is
unspecified: those are in the fixture for the loss value only).  ``cases`` holds (P, C, ignored per mille, per_image, ties, ndim)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _lovasz_reference as lref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g20_lovasz.npz")
IGNORE = 255
# (name, P or (B, H, W), C, ignored share, kind)
CASES = (("p17", 17, 2, 0.0, "random"), ("p64", 64, 3, 0.2, "random"), ("p257", 257, 5, 0.5, "random"),
         ("p1000", 1000, 10, 0.9, "random"), ("p4097", 4097, 16, 0.2, "random"), ("absent", 257, 5, 0.0, "absent"),
         ("single", 64, 3, 0.2, "single"), ("images", (3, 7, 9), 5, 0.2, "random"), ("dup4", 64, 3, 0.2, "dup4"),
         ("half", 32, 2, 0.0, "half"))


def _load(ref):
    try:
        import torchvision  # noqa: F401
    except ImportError:
        sys.modules["torchvision"] = types.ModuleType("torchvision")
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(ref, "mopa", "common", "utils", "loss.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.lovasz_softmax


def inputs(k):
    """-> (p float32, y int64, per_image, ties) of case k; seeded, independent of the reference."""
    name, shape, C, share, kind = CASES[k]
    rng = np.random.Generator(np.random.PCG64(20000 + 100 * k))
    per_image = isinstance(shape, tuple)
    P = int(np.prod(shape))
    rows = P // 4 if kind == "dup4" else P
    z = torch.from_numpy((3.0 * rng.standard_normal((rows, C))).astype(np.float32))
    p = torch.softmax(z, 1).numpy()
    y = rng.integers(0, C, rows)
    if kind == "absent":
        y[y == 3] = 1
    if kind == "single":
        y[:] = 1
    if kind == "dup4":
        p, y = np.tile(p, (4, 1)), np.tile(y, 4)
    if kind == "half":
        p = np.full((P, 2), 0.5, np.float32)
    y = np.where(rng.random(P) < share, IGNORE, y).astype(np.int64)
    if per_image:
        B, H, W = shape
        p = np.ascontiguousarray(p.reshape(B, H, W, C).transpose(0, 3, 1, 2))
        y = y.reshape(B, H, W)
    return np.ascontiguousarray(p, np.float32), y, per_image, kind in ("dup4", "half")


def main():
    lovasz_softmax = _load(sys.argv[1])
    save, rows = {}, []
    for k, (name, shape, C, share, kind) in enumerate(CASES):
        p, y, per_image, ties = inputs(k)
        t = torch.from_numpy(p).requires_grad_(True)
        loss = lovasz_softmax(t, torch.from_numpy(y), classes="present", per_image=per_image, ignore=IGNORE)
        grad, = torch.autograd.grad(loss, t)
        assert loss.dtype == torch.float32 and grad.dtype == torch.float32
        ref_loss, ref_grad = float(loss.detach()), grad.numpy()
        if per_image:
            p2, y2, off = lref.from_nchw(p, y)
            r = lref.lovasz(p2, y2, ignore=IGNORE, offsets=off)
            g = r["grad"].reshape(p.shape[0], p.shape[2], p.shape[3], C).transpose(0, 3, 1, 2)
        else:
            r = lref.lovasz(p, y, ignore=IGNORE)
            g = r["grad"]
        loss_err = abs(r["loss"] - ref_loss) / abs(ref_loss)
        grad_err = np.nan if ties else np.abs(g - ref_grad).max() / np.abs(ref_grad).max()
        save[f"c{k}_p"], save[f"c{k}_y"] = p, y
        save[f"c{k}_loss"], save[f"c{k}_grad"] = np.float32(ref_loss), ref_grad
        save[f"c{k}_loss_err"], save[f"c{k}_grad_err"] = np.float64(loss_err), np.float64(grad_err)
        rows.append((int(np.prod(shape)), C, int(round(1000 * share)), int(per_image), int(ties), p.ndim))
        print(name, "loss", ref_loss, "restatement: loss rel %.2e grad / max|grad| %.2e" % (loss_err, grad_err))
    save["cases"] = np.asarray(rows, np.int64)
    np.savez_compressed(OUT, **save)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    le = max(float(save[f"c{k}_loss_err"]) for k in range(len(CASES)))
    ge = np.nanmax([float(save[f"c{k}_grad_err"]) for k in range(len(CASES))])
    print("worst: loss %.3e grad %.3e  -> bounds of tests/test_lovasz_host.py: %.3e %.3e" % (le, ge, 4 * le, 4 * ge))


if __name__ == "__main__":
    main()
