"""numpy float64 restatement of the reference's SupConLoss (mopa/models/losses.py:123-184) with both gradients, and of l2_norm
(mopa/common/utils/loss.py:230-238) with its gradient, from float32 inputs -- the yardstick of tests/test_gpu_supcon.py, itself held
against the reference's float64 autograd by tests/test_supcon_host.py (tests/golden/g21_supcon.npz).

With S = A Q^T / T, per anchor i: m_i = max_j S_ij (a constant of the gradient), P_i = {j : la_i == lq_j}, N_i the rest, n_i = |P_i|,
D_i = sum_{N_i} (exp(S_ij - m_i) + eps) = E_i + eps |N_i|, mlpp_i = (1 / n_i) sum_{P_i} (S_ij - m_i) - log D_i, loss = -mean_i mlpp_i;
G_ij = -(1 / divisor) ([j in P_i] / n_i - [j in N_i] exp(S_ij - m_i) / D_i), dA = G Q / T, dQ = G^T A / T.  A row with n_i = 0 or
|N_i| = 0 is invalid: the default mode gives a NaN loss and all-NaN gradients, ``skip_invalid`` leaves such rows out of the sum and
divides by the number of valid rows (none: 0 and zero gradients).  Everything is row-blocked: no more than BLOCK_BYTES at a time."""
import numpy as np

EPS32 = float(np.float32(1e-5))      # what the reference's float32 path adds per negative pair
L2_EPS = float(np.float32(1e-8))     # torch.Tensor([1e-8]) is a float32 tensor
BLOCK_BYTES = 4 << 20
U = 2.0 ** -24                       # unit roundoff of float32


def _blocks(Na, per_row_bytes):
    step = max(1, int(BLOCK_BYTES // max(1, per_row_bytes)))
    return [(s, min(s + step, Na)) for s in range(0, Na, step)]


def supcon(la, A, Q, lq, T=0.1, eps=EPS32, skip_invalid=False, g=1.0, bounds=False, defect=None):
    """-> dict(loss, dA, dQ, status, valid); with ``bounds`` also loss_bound, dA_bound, dQ_bound (see tests/test_gpu_supcon.py) for
    the device's arithmetic.  ``defect``: one-defect variants for the mutation tests of tests/test_supcon_host.py."""
    A = np.asarray(A, np.float64)
    Q = np.asarray(Q, np.float64)
    la = np.asarray(la).reshape(-1).astype(np.int64)
    lq = np.asarray(lq).reshape(-1).astype(np.int64)
    Na, F = A.shape
    Nq = Q.shape[0]
    T = float(T)
    m = np.empty(Na)
    D = np.empty(Na)
    n = np.empty(Na)
    nn = np.empty(Na)
    mlpp = np.empty(Na)
    blocks = _blocks(Na, Nq * 8 * 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s, e in blocks:
            S = A[s:e] @ Q.T / T
            P = la[s:e, None] == lq[None, :]
            if defect == "self_excluded" and Na == Nq:
                P = P & ~np.eye(Na, dtype=bool)[s:e]
            mb = S.max(1)
            ex = np.exp(S - mb[:, None])
            if defect == "all_in_denominator":
                Db = (ex + eps).sum(1)
            else:
                Db = np.where(P, 0.0, ex).sum(1) + (0.0 if defect == "no_eps" else eps) * (~P).sum(1)
            nb = P.sum(1).astype(np.float64)
            m[s:e], D[s:e], n[s:e], nn[s:e] = mb, Db, nb, (~P).sum(1)
            mlpp[s:e] = np.where(P, S - mb[:, None], 0.0).sum(1) / nb - np.log(Db)
    valid = (n > 0) & (nn > 0)
    status = (1 if (n == 0).any() else 0) | (2 if (nn == 0).any() else 0)
    if skip_invalid:
        div = float(valid.sum())
        loss = -mlpp[valid].sum() / div if div else 0.0
        scale = 1.0 / div if div else 0.0
    elif not valid.all():
        loss, scale = np.nan, np.nan
    else:
        loss, scale = -mlpp.sum() / Na, 1.0 / Na
    out = {"loss": float(loss), "status": status, "valid": valid, "m": m, "D": D, "n": n}
    dA = np.zeros((Na, F))
    dQ = np.zeros((Nq, F))
    if bounds:
        bA, bQ, vQ, var = np.zeros((Na, F)), np.zeros((Nq, F)), np.zeros((Nq, F)), 0.0
        L = -(-Nq // 64)
        per_row = Nq * 8 * (4 + F)
    else:
        per_row = Nq * 8 * 4
    if np.isnan(scale):
        dA[:], dQ[:] = np.nan, np.nan
    else:
        for s, e in _blocks(Na, per_row):
            S = A[s:e] @ Q.T / T
            P = la[s:e, None] == lq[None, :]
            if defect == "self_excluded" and Na == Nq:
                P = P & ~np.eye(Na, dtype=bool)[s:e]
            keep = valid[s:e] if skip_invalid else np.ones(e - s, bool)
            with np.errstate(divide="ignore", invalid="ignore"):
                ex = np.exp(S - m[s:e, None]) / D[s:e, None]
                W = np.where(P, 1.0 / n[s:e, None], 0.0) - (ex if defect == "all_in_denominator" else np.where(P, 0.0, ex))
            W = np.where(keep[:, None], W, 0.0)
            c = -g * scale / T
            dA[s:e] = c * (W @ Q)
            dQ += c * (W.T @ A[s:e])
            if bounds:
                # sigma2_ij: variance of the device's S_ij (and, for a negative pair, of its exponent S_ij - m_i) under the model of
                # the docstring of tests/test_gpu_supcon.py: every rounding is an independent error, uniform in +-u |rounded value|
                part2 = (np.cumsum(A[s:e, None, :] * Q[None, :, :], axis=2) ** 2).sum(2)
                sig2 = (U * U / 3.0) * (part2 / (T * T) + S * S + np.where(P, 0.0, (S - m[s:e, None]) ** 2 + 4.0))   # + 4: expf, 1 ulp = 2 u
                aW = np.abs(W)
                EoD = np.where(keep, np.where(P, 0.0, ex).sum(1), 0.0)                      # E_i / D_i
                smaxP = np.where(P, np.abs(S), 0.0).max(1)
                var_sums = (U * U / 3.0) * ((2 * L + 6) * EoD ** 2 + (L * L * smaxP ** 2 / np.maximum(n[s:e], 1) if L > 1 else 0.0))
                var += float((((aW * scale) ** 2 * sig2).sum(1) + keep * scale ** 2 * var_sums).sum())
                # the error of log D_i, common to the negatives of a row: six sigma
                dlogD = 6.0 * np.sqrt((np.where(P, 0.0, aW) ** 2 * sig2).sum(1) + (U * U / 3.0) * (2 * L + 6))
                common = dlogD[:, None] * np.where(P, 0.0, aW) + 4.0 * U * aW
                chainA = 6.0 * np.sqrt((Nq + 64.0) / 3.0) * U
                chainQ = 6.0 * np.sqrt((Na + 64.0) / 3.0) * U
                absQ, absA = np.abs(Q), np.abs(A[s:e])
                bA[s:e] = abs(c) * (6.0 * np.sqrt((aW ** 2 * sig2) @ absQ ** 2) + (common + chainA * aW) @ absQ)
                vQ += (aW ** 2 * sig2).T @ absA ** 2
                bQ += abs(c) * ((common + chainQ * aW).T @ absA)
        if bounds:
            out["loss_bound"] = 6.0 * np.sqrt(var) + 1e-13
            out["dA_bound"] = bA + U * np.abs(dA) + 1e-30
            out["dQ_bound"] = bQ + abs(c) * 6.0 * np.sqrt(vQ) + U * np.abs(dQ) + 1e-30
    out["dA"], out["dQ"] = dA, dQ
    return out


def l2_norm(x, g=None):
    """-> (y, dx or None): y = x / where(norm > eps, norm, eps); dx = (g - y (y . g)) / norm above eps, g / eps at or below it."""
    x = np.asarray(x, np.float64)
    norm = np.sqrt((x * x).sum(1))
    above = norm > L2_EPS
    den = np.where(above, norm, L2_EPS)
    y = x / den[:, None]
    if g is None:
        return y, None
    g = np.asarray(g, np.float64)
    dx = np.where(above[:, None], (g - y * (y * g).sum(1, keepdims=True)) / den[:, None], g / L2_EPS)
    return y, dx


def unit_rows(rng, N, F):
    x = rng.standard_normal((N, F))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def labels_with_both(rng, Na, Nq, classes):
    """Labels such that every anchor has a positive and a negative in the pool (every class appears in the pool, at least two do)."""
    lq = rng.integers(0, classes, Nq)
    lq[:classes] = np.arange(classes)[:Nq]
    la = rng.integers(0, min(classes, Nq), Na)
    return la.astype(np.int64), lq.astype(np.int64)
