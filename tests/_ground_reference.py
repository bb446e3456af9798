"""The ground estimate of mopa_amd/ground.py restated in float64 numpy: the yardstick of tests/test_ground_host.py and
tests/test_gpu_ground.py.  It is the published Patchwork core as DESIGN.md section 4 states it -- concentric zones, a plane fitted
per patch from the lowest points, three likelihood tests -- and NOT Patchwork++ (no adaptive thresholds, no reflected-noise removal
beyond the zone-0 cut, no vertical-plane fitting, no temporal revert).

``estimate(points, sensor_height)`` returns the mask and, per point, a "fragile" flag: the point's result hangs on a comparison
that the last bits of another summation order, another atan2 / sqrt or another eigen-solver could turn.  Inputs are float32 held
exactly in float64 and both sides accumulate in float64, so on coordinates up to 80 m those differences stay several orders below
the margins used here (1e-9 relative on the bin boundaries, 1e-6 absolute on every threshold).  A comparison of another
implementation with this one leaves the fragile points out and caps their share.
"""
import numpy as np

RINGS = (2, 4, 4, 4)
SECTORS = (16, 32, 54, 32)
ZONE_PATCH0 = (0, 32, 160, 376)          # first patch of a zone: zone-major, then ring, then sector
ZONE_RING0 = (0, 2, 6, 10)               # first global ring index of a zone
N_PATCHES = 504
DEFAULTS = dict(rmin=2.7, rmax=80.0, num_min_pts=10, num_lpr=20, num_iter=3, th_seeds=0.125, th_dist=0.125, uprightness=0.707,
                elevation=(0.523, 0.746, 0.879, 1.125), flatness=(0.0005, 0.000725, 0.001, 0.001), noise_cut=1.1)
REL = 1e-9                               # bin boundaries
ABS = 1e-6                               # thresholds and decision quantities
GAP = 1e-6                               # lambda1 - lambda0 <= GAP * lambda2: the normal is not determined


def zone_bounds(rmin, rmax):
    return np.array([rmin, (7 * rmin + rmax) / 8, (3 * rmin + rmax) / 4, (rmin + rmax) / 2, rmax], np.float64)


def _near(v, b, rel=REL):
    return np.abs(v - b) <= rel * np.abs(b)


def patch_ids(points, sensor_height, **kw):
    """-> (patch id (N,) int64, -1 = in no patch; fragile (N,) bool: r, theta or z within the margins of a boundary)."""
    prm = dict(DEFAULTS, **kw)
    P = np.asarray(points)[:, :3].astype(np.float64)
    n = P.shape[0]
    pid = np.full(n, -1, np.int64)
    fragile = np.zeros(n, bool)
    if n == 0:
        return pid, fragile
    finite = np.isfinite(P).all(1)
    x, y, z = (np.where(finite, P[:, k], 0.0) for k in range(3))
    r = np.sqrt(x * x + y * y)
    th = np.arctan2(y, x)
    th = np.where(th < 0, th + 2 * np.pi, th)
    b = zone_bounds(prm["rmin"], prm["rmax"])
    inside = finite & (r >= b[0]) & (r < b[4])
    zone = np.clip(np.searchsorted(b, r, side="right") - 1, 0, 3)
    cut = -prm["noise_cut"] * sensor_height
    for k in range(4):
        sel = inside & (zone == k)
        rw = (b[k + 1] - b[k]) / RINGS[k]
        sa = 2 * np.pi / SECTORS[k]
        ring = np.minimum(((r - b[k]) / rw).astype(np.int64), RINGS[k] - 1)
        sector = np.minimum((th / sa).astype(np.int64), SECTORS[k] - 1)
        ids = ZONE_PATCH0[k] + ring * SECTORS[k] + sector
        if k == 0:
            fragile |= sel & (np.abs(z - cut) <= ABS)
            sel = sel & ~(z < cut)
        pid[sel] = ids[sel]
        # the zone's own boundaries: its ring edges (the outer one is the next zone's first) and its sector edges
        zsel = finite & (zone == k)
        for j in range(RINGS[k] + 1):
            fragile |= zsel & _near(r, b[k] + j * rw)
        for j in range(1, SECTORS[k] + 1):
            fragile |= zsel & _near(th, j * sa)
    fragile |= finite & (_near(r, b[0]) | _near(r, b[4]))
    return pid, fragile


def patch_table():
    """(504, 3) [zone, ring, sector] of every patch id, by brute force."""
    return np.array([(k, ring, s) for k in range(4) for ring in range(RINGS[k]) for s in range(SECTORS[k])], np.int64)


def _fit(S):
    """Plane through the (m, 3) set: mean, eigenvalues ascending, upward normal, and whether the normal is determined."""
    mu = S.mean(0)
    d = S - mu
    cov = d.T @ d / (S.shape[0] - 1)
    lam, vec = np.linalg.eigh(cov)
    nrm = vec[:, 0]
    if nrm[2] < 0:
        nrm = -nrm
    return mu, lam, nrm, bool(lam[1] - lam[0] <= GAP * lam[2])


def fit_patch(Q, g, sensor_height, prm):
    """One patch of (n, 3) float64 points in global ring g -> (ground (n,) bool, fragile (n,) bool)."""
    n = Q.shape[0]
    ground = np.zeros(n, bool)
    fragile = np.zeros(n, bool)
    if n < prm["num_min_pts"]:
        return ground, fragile
    z = Q[:, 2]
    lpr = np.sort(z)[:min(prm["num_lpr"], n)].mean()
    cur = z < lpr + prm["th_seeds"]
    fragile |= np.abs(z - (lpr + prm["th_seeds"])) <= ABS
    whole = False                                   # a quantity of the whole patch is within the margins
    for _ in range(prm["num_iter"]):
        if cur.sum() < 3:
            fragile[:] |= whole
            return ground, fragile
        mu, lam, nrm, loose = _fit(Q[cur])
        whole |= loose
        dist = Q @ nrm - nrm @ mu
        fragile |= np.abs(dist - prm["th_dist"]) <= ABS
        cur = dist < prm["th_dist"]
    if cur.sum() < 3:
        fragile[:] |= whole
        return ground, fragile
    mu, lam, nrm, loose = _fit(Q[cur])
    whole |= loose
    up = nrm[2] - prm["uprightness"]
    whole |= abs(up) <= ABS
    ok = up >= 0
    if g < 4:
        elev = mu[2] - (-sensor_height + prm["elevation"][g])
        whole |= abs(elev) <= ABS
        if elev > 0 or abs(elev) <= ABS:
            with np.errstate(invalid="ignore", divide="ignore"):
                flat = lam[0] / (lam[0] + lam[1] + lam[2]) - prm["flatness"][g]
            whole |= bool(abs(flat) <= ABS)
            if elev > 0:
                ok = ok and bool(flat < 0)
    if ok:
        ground = cur
    fragile[:] |= whole
    return ground, fragile


def estimate(points, sensor_height, **kw):
    """-> (mask (N,) uint8, fragile (N,) bool) of one scan."""
    prm = dict(DEFAULTS, **kw)
    P = np.asarray(points)[:, :3].astype(np.float64)
    pid, fragile = patch_ids(points, sensor_height, **kw)
    mask = np.zeros(P.shape[0], np.uint8)
    order = np.argsort(pid, kind="stable")
    sorted_pid = pid[order]
    lo = np.searchsorted(sorted_pid, np.arange(N_PATCHES), side="left")
    hi = np.searchsorted(sorted_pid, np.arange(N_PATCHES), side="right")
    ring_of = np.concatenate([ZONE_RING0[k] + np.repeat(np.arange(RINGS[k]), SECTORS[k]) for k in range(4)])
    for p in range(N_PATCHES):
        if hi[p] - lo[p] == 0:
            continue
        idx = order[lo[p]:hi[p]]
        g, f = fit_patch(P[idx], int(ring_of[p]), sensor_height, prm)
        mask[idx] = g
        fragile[idx] |= f
    return mask, fragile
