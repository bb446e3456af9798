"""numpy float64 restatement of the reference's ``logcoral_loss`` (mopa/models/losses.py:47-93) and of its gradient -- the yardstick
of tests/test_coral_host.py (held against the reference's own fp64 autograd through tests/golden/g19_logcoral.npz) and of
tests/test_gpu_coral.py.  TEST INFRASTRUCTURE ONLY.

Forward, quirks included: ``batch_size`` is the FIRST dimension before flattening, ``factor = 1 / (batch_size - 1)`` scales BOTH
covariances, each (N, F) matrix is centred by its own column means, a covariance entry > 1e30 or NaN on either side turns both
covariances into the identity, L = V diag(log|lambda|) V^T from the symmetric eigendecomposition (what the reference's SVD gives for
a symmetric positive semi-definite matrix), loss = mean((L_src - L_trg)^2).

Backward: D = L_src - L_trg, G = 2 D / F^2, per side dC = V [(V^T (+-G) V) o K] V^T with the divided differences
K_ij = (log l_i - log l_j) / (l_i - l_j), taken as log1p((a - b) / b) / (a - b) for a = max, b = min (the same number without the
cancellation of two logarithms), and the limit 2 / (l_i + l_j) where |l_i - l_j| <= 1e-9 max(l_i, l_j); dX = factor Xc (dC + dC^T).
"""
import numpy as np

EQUAL_RTOL = 1e-9


def _flatten(x):
    x = np.asarray(x, np.float64)
    return x.reshape(-1, x.shape[-1])


def divided_differences(lam):
    """K of the matrix logarithm at the eigenvalues |lam| (F,) -> (F, F)."""
    e = np.abs(np.asarray(lam, np.float64))
    a, b = np.maximum(e[:, None], e[None, :]), np.minimum(e[:, None], e[None, :])
    d = a - b
    equal = d <= EQUAL_RTOL * a
    with np.errstate(divide="ignore", invalid="ignore"):
        K = np.where(equal, 2.0 / (a + b), np.log1p(d / b) / np.where(equal, 1.0, d))
    return K


def logcoral(x_src, x_trg, grad=True):
    """-> dict(loss, d_src, d_trg, guard, cond): float64 loss and gradients in the inputs' shapes."""
    shape_s, shape_t = np.shape(x_src), np.shape(x_trg)
    if shape_s[-1] != shape_t[-1] or len(shape_s) < 2:
        raise ValueError("logcoral: feature widths differ or an input has fewer than two dimensions")
    factor = 1.0 / (shape_s[0] - 1)
    F = shape_s[-1]
    xs, xt = _flatten(x_src), _flatten(x_trg)
    with np.errstate(all="ignore"):
        cs, ct = xs - xs.mean(0), xt - xt.mean(0)
        covs = [factor * (c.T @ c) for c in (cs, ct)]
        guard = bool(any((c > 1e30).any() or np.isnan(c).any() for c in covs))
    if guard:
        return {"loss": 0.0, "d_src": np.zeros(shape_s), "d_trg": np.zeros(shape_t), "guard": True, "cond": 1.0}
    eig = []
    for c in covs:
        lam, V = np.linalg.eigh((c + c.T) / 2)
        eig.append((lam, V))
    with np.errstate(divide="ignore"):
        Ls = [(V * np.log(np.abs(lam))) @ V.T for lam, V in eig]
    D = Ls[0] - Ls[1]
    out = {"loss": float(np.mean(D * D)), "guard": False,
           "cond": max(float(np.abs(lam).max() / np.abs(lam).min()) if np.abs(lam).min() > 0 else np.inf for lam, _ in eig)}
    if grad:
        G = 2.0 * D / (F * F)
        for key, sign, (lam, V), xc, shape in (("d_src", 1.0, eig[0], cs, shape_s), ("d_trg", -1.0, eig[1], ct, shape_t)):
            dC = V @ ((V.T @ (sign * G) @ V) * divided_differences(lam)) @ V.T
            out[key] = (factor * xc @ (dC + dC.T)).reshape(shape)
    return out


def mixed_gaussian(rng, n, f, offset=0.0):
    """Gaussian rows times a random mixing matrix (condition numbers of the covariance stay at or below ~1e7 for the shapes the tests
    use), plus `offset` column standard deviations added to every column; float32."""
    mix = rng.standard_normal((f, f))
    x = rng.standard_normal((n, f)) @ mix
    x = x + offset * x.std(0, keepdims=True)
    return x.astype(np.float32)


COND_MAX = 1e7   # beyond it two float64 evaluations no longer agree to the 1e-8 the tests ask of the gradient


def conditioned_pair(seed, ns, nt, f, offset=0.0, shape_src=None, shape_trg=None):
    """(x_src, x_trg) from the first of the seeds seed, seed + 1, ... whose covariances both have a condition number <= COND_MAX."""
    for j in range(100):
        rng = np.random.Generator(np.random.PCG64(seed + j))
        xs, xt = mixed_gaussian(rng, ns, f, offset), mixed_gaussian(rng, nt, f, offset)
        xs, xt = (xs.reshape(shape_src) if shape_src else xs), (xt.reshape(shape_trg) if shape_trg else xt)
        if logcoral(xs, xt, grad=False)["cond"] <= COND_MAX:
            return xs, xt
    raise RuntimeError("no draw within the condition bound")


def guard_threshold_pair(x_src, x_trg, target=3e30):
    """The inputs scaled (float32) so that the largest covariance entry under factor = 1 / (x_src.shape[0] - 1) is `target`."""
    factor = 1.0 / (np.shape(x_src)[0] - 1)
    top = 0.0
    for x in (x_src, x_trg):
        c = _flatten(x)
        c = c - c.mean(0)
        top = max(top, factor * (c * c).sum(0).max())
    s = np.float32(np.sqrt(target / top))
    return np.asarray(x_src, np.float32) * s, np.asarray(x_trg, np.float32) * s
