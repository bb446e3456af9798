"""Generate tests/golden/g12_minent.npz by RUNNING the reference's ``entropy_loss`` (mopa/models/losses.py:21-34) on the softmax of
seeded logits, as ``train_xmuda.py:323-330`` calls it (``entropy_loss(F.softmax(seg_logit, dim=1))``).  The module is loaded by
path from the checkout; its import of ``mopa.models.xmuda_arch`` (for ``batch_segment``, which ``entropy_loss`` does not use) is
answered by a stub module.

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixture is what travels).
Usage, from the repo root:  python tests/golden_gen/g12_minent.py PATH_TO_MOPA_CHECKOUT

Per case ``k`` the .npz holds ``c<k>_z`` (float32 logits ~ N(0, 2); row 0 saturated: (120, 0, ..., 0)), ``c<k>_loss32`` /
``c<k>_loss64`` (the reference's value on the float32 / float64 logits) and ``c<k>_grad32`` / ``c<k>_grad64`` (its autograd gradient
with respect to the logits); ``cases`` holds the (N, C) list.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "g12_minent.npz")
CASES = ((63, 2), (257, 5), (1000, 11), (4099, 10))


def _load(ref):
    stub = types.ModuleType("mopa.models.xmuda_arch")
    stub.batch_segment = lambda *a, **k: None
    for name in ("mopa", "mopa.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["mopa.models.xmuda_arch"] = stub
    spec = importlib.util.spec_from_file_location("ref_losses", os.path.join(ref, "mopa", "models", "losses.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.entropy_loss


def logits(N, C):
    rng = np.random.Generator(np.random.PCG64(12000 + 100 * C + N % 9973))
    z = rng.standard_normal((N, C), dtype=np.float32) * 2
    z[0] = 0
    z[0, 0] = 120
    return z


def main():
    entropy_loss = _load(sys.argv[1])
    save = {"cases": np.asarray(CASES, np.int64)}
    for k, (N, C) in enumerate(CASES):
        z = logits(N, C)
        save[f"c{k}_z"] = z
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            t = torch.from_numpy(z).to(dt).requires_grad_(True)
            loss = entropy_loss(F.softmax(t, dim=1))
            (grad,) = torch.autograd.grad(loss, t)
            assert torch.isfinite(loss) and torch.isfinite(grad).all()
            save[f"c{k}_loss{tag}"] = loss.detach().numpy()
            save[f"c{k}_grad{tag}"] = grad.numpy()
        l32, l64 = float(save[f"c{k}_loss32"]), float(save[f"c{k}_loss64"])
        g32, g64 = save[f"c{k}_grad32"].astype(np.float64), save[f"c{k}_grad64"]
        print((N, C), "loss", l64, "fp32 rel err", abs(l32 - l64) / abs(l64), "grad fp32 err / max|grad|",
              np.abs(g32 - g64).max() / np.abs(g64).max())
    np.savez_compressed(OUT, **save)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
