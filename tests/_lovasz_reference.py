"""Numpy restatement of the Lovasz-softmax arithmetic of DESIGN.md section 4 (csrc/lovasz.hip), the yardstick of the device tests.

The key e = |fg - p| is ONE float32 operation (the reference's expression, the same bits); the order is a stable descending argsort
(equal keys in ascending row order); everything behind the sort is float64.  tests/test_lovasz_host.py holds this file to the
reference's own result (tests/golden/g20_lovasz.npz).

``defect`` (tests only) plants one mistake: 'ascending', 'no_difference', 'mean_over_C', 'keep_ignored'."""
import numpy as np


def _selected(classes, C, counts):
    if isinstance(classes, str):
        if classes == "all":
            return list(range(C))
        if classes == "present":
            return [c for c in range(C) if counts[c] > 0]
        raise ValueError(classes)
    return [int(c) for c in classes]


def _flat(p, y, classes, ignore, defect):
    """One segment -> (loss, d loss / d p) in float64."""
    P, C = p.shape
    grad = np.zeros((P, C), np.float64)
    valid = np.ones(P, bool) if (ignore is None or defect == "keep_ignored") else (y != ignore)
    rows = np.nonzero(valid)[0]
    V = len(rows)
    if V == 0:
        return 0.0, grad
    yv = y[rows]
    counts = [int((yv == c).sum()) for c in range(C)]
    sel = _selected(classes, C, counts)
    if not sel:
        return 0.0, grad
    n_mean = C if defect == "mean_over_C" else len(sel)
    total = 0.0
    for c in sel:
        fg = (yv == c)
        pc = p[rows, c]
        e = np.abs(fg.astype(np.float32) - pc)                      # float32, one operation
        assert e.dtype == np.float32
        order = np.argsort(e if defect == "ascending" else -e, kind="stable")
        es = e[order].astype(np.float64)
        fgs = fg[order].astype(np.int64)
        G = int(fgs.sum())
        cum = np.cumsum(fgs)
        k1 = np.arange(1, V + 1, dtype=np.int64)
        J = 1.0 - (G - cum).astype(np.float64) / (G + (k1 - cum)).astype(np.float64)
        w = J.copy()
        if defect != "no_difference":
            w[1:] = J[1:] - J[:-1]
        total += float(np.sum(es * w))
        sign = np.where(es == 0.0, 0.0, np.where(fgs == 1, -1.0, 1.0))   # sign(p - fg)
        grad[rows[order], c] = sign * w / n_mean
    return total / n_mean, grad


def lovasz(p, y, classes="present", ignore=None, offsets=None, defect=None):
    """p (P, C) float32, y (P,) integers -> {'loss': float, 'grad': (P, C) float64 d loss / d p}; ``offsets``: S + 1 row offsets of the
    segments (the mean over segments; a segment with nothing selected contributes 0 and counts)."""
    p = np.ascontiguousarray(p)
    assert p.dtype == np.float32 and p.ndim == 2
    y = np.asarray(y).astype(np.int64)
    P = p.shape[0]
    offsets = [0, P] if offsets is None else [int(o) for o in offsets]
    S = len(offsets) - 1
    grad = np.zeros(p.shape, np.float64)
    loss = 0.0
    for s in range(S):
        a, b = offsets[s], offsets[s + 1]
        l, g = _flat(p[a:b], y[a:b], classes, ignore, defect)
        loss += l
        grad[a:b] = g
    return {"loss": loss / S, "grad": grad / S}


def logits_grad(p, dp):
    """d loss / d logits in float64, given the float32 probabilities p = softmax(z) and d loss / d p."""
    p64 = p.astype(np.float64)
    return p64 * (dp - (dp * p64).sum(axis=1, keepdims=True))


def from_nchw(probas, labels):
    """(B, C, H, W), (B, H, W) -> (B H W, C), (B H W,), offsets of the B images."""
    B, C, H, W = probas.shape
    return (np.ascontiguousarray(probas.transpose(0, 2, 3, 1)).reshape(-1, C), np.asarray(labels).reshape(-1),
            [b * H * W for b in range(B + 1)])


def softmax32(z):
    z = z.astype(np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
