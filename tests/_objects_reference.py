"""A numpy restatement of what mopa_amd/objects.py computes (csrc/objects.hip), and the cases that the host
and the device tests share.  Brute force and float64 throughout: the full distance matrix, no grid, no union-find.

Labels of one segment (the points of one class in one scan, in row order) are those of
``sklearn.cluster.DBSCAN(eps, min_samples).fit_predict``:
  * d2(i, j) = (dx dx + dy dy) + dz dz in float64 from the float32 coordinates; j is a neighbour of i iff d2 <= eps * eps (i is its
    own neighbour; d == eps counts);
  * i is core iff it has at least min_samples neighbours;
  * the clusters are the connected components of the core points under the neighbour relation, numbered 0, 1, ... by their
    lowest-index core point;
  * a point that is not core takes the lowest cluster number among its core neighbours, or -1 (noise) without one.
Rows of a requested class with a non-finite coordinate or |coordinate| / eps >= 2^20 are in no segment (label -2) and counted.
Instances: per (scan, class position) the values of np.unique over the segment's labels (the noise group -1 first, left out when
include_noise is False); the float32 range sqrt(x x + y y + z z + 1e-5) per point, its float64 mean per instance, keep = mean <=
max_distance.  ``extract`` asserts that every mean stays 1e-3 max_distance away from max_distance, so that keep cannot hinge on the
order of a sum."""
import numpy as np

F32 = np.float32
EPS, MIN_SAMPLES, MAX_DISTANCE = 4.0, 5, 15.0


# ------------------------------------------------------------------------------------------------ the labels of one segment
def dbscan_labels(X, eps=EPS, min_samples=MIN_SAMPLES):
    X = np.asarray(X, F32)[:, :3].astype(np.float64)
    n = len(X)
    lab = np.full(n, -1, np.int64)
    if n == 0:
        return lab
    d = X[:, None, 0] - X[None, :, 0]
    d2 = d * d
    d = X[:, None, 1] - X[None, :, 1]
    d2 = d2 + d * d
    d = X[:, None, 2] - X[None, :, 2]
    d2 = d2 + d * d
    adj = d2 <= np.float64(eps) * np.float64(eps)
    del d, d2
    core = adj.sum(1) >= min_samples
    cid = 0
    for i in np.nonzero(core)[0]:
        if lab[i] >= 0:
            continue
        members = np.zeros(n, bool)
        members[i] = True
        frontier = members.copy()
        while frontier.any():
            reach = adj[frontier].any(0) & core & ~members
            members |= reach
            frontier = reach
        lab[members] = cid
        cid += 1
    for i in np.nonzero(~core)[0]:
        near = lab[adj[i] & core]
        if near.size:
            lab[i] = near.min()
    return lab


def point_range(P):
    P = np.asarray(P, F32)
    return np.sqrt(P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1] + P[:, 2] * P[:, 2] + F32(0.00001))


def accepted(P, eps=EPS):
    P = np.asarray(P, F32)[:, :3]
    with np.errstate(invalid="ignore"):
        return np.isfinite(P).all(1) & (np.abs(P.astype(np.float64) / np.float64(eps)) < 2.0 ** 20).all(1)


# ------------------------------------------------------------------------------------------------ the whole call
def extract(point_sets, label_sets, class_ids, eps=EPS, min_samples=MIN_SAMPLES, max_distance=MAX_DISTANCE, include_noise=True):
    """-> dict(labels [B x (N_b,) int32], table (M, 4) int32, offsets (M + 1,) int32, mean_range (M,) float64, keep (M,) uint8,
    points (total, cols) float32, n_rejected)."""
    cols = point_sets[0].shape[1]
    labels, table, offsets, means, keep, points, n_rejected = [], [], [0], [], [], [], 0
    for b, (P, L) in enumerate(zip(point_sets, label_sets)):
        P, L = np.asarray(P, F32), np.asarray(L).astype(np.int64)
        out = np.full(len(P), -2, np.int32)
        ok = accepted(P, eps)
        for c, cid in enumerate(class_ids):
            of_class = L == cid
            n_rejected += int((of_class & ~ok).sum())
            rows = np.nonzero(of_class & ok)[0]
            if rows.size == 0:
                continue
            lab = dbscan_labels(P[rows], eps, min_samples)
            out[rows] = lab
            rng = point_range(P[rows]).astype(np.float64)
            for inst in np.unique(lab).tolist():
                if inst == -1 and not include_noise:
                    continue
                sel = lab == inst
                mean = float(np.sum(rng[sel]) / sel.sum())
                assert abs(mean - max_distance) >= 1e-3 * max_distance, f"scan {b} class {cid} instance {inst}: mean range {mean} too close to {max_distance}"
                table.append((b, c, inst, int(sel.sum())))
                offsets.append(offsets[-1] + int(sel.sum()))
                means.append(mean)
                keep.append(mean <= max_distance)
                points.append(P[rows[sel]])
        labels.append(out)
    return dict(labels=labels, table=np.asarray(table, np.int32).reshape(-1, 4), offsets=np.asarray(offsets, np.int32),
                mean_range=np.asarray(means, np.float64), keep=np.asarray(keep, np.uint8),
                points=np.concatenate(points, 0) if points else np.zeros((0, cols), F32), n_rejected=n_rejected)


# ------------------------------------------------------------------------------------------------ the bank
def capped(ref, n_classes, max_num):
    """The instances a bank takes from one ``extract`` result, per class position: kept ones in table order while the class holds
    fewer than max_num.  -> [list of (n, cols) arrays per class position]."""
    out = [[] for _ in range(n_classes)]
    for i, (b, c, inst, n) in enumerate(ref["table"].tolist()):
        if ref["keep"][i] and len(out[c]) < max_num:
            out[c].append(ref["points"][ref["offsets"][i]:ref["offsets"][i + 1]])
    return out


def obj_sampling(files, label_value, cols):
    """What the datasets' obj_sampling does with the sorted file list of a class."""
    k = np.random.choice(len(files), 1)
    obj_pc = np.fromfile(files[k[0]], dtype=F32).reshape((-1, cols))
    assert not np.any(np.isnan(obj_pc))
    return obj_pc, np.ones(obj_pc.shape[0]) * label_value


# ------------------------------------------------------------------------------------------------ the shared cases
def _blob(rng, n, centre, spread):
    return (np.asarray(centre, np.float64) + rng.normal(0.0, spread, (n, 3))).astype(F32)


def _chain(rng, nodes=300, step=3.9):
    """2 points per node, the nodes `step` apart along a line that drifts through y and z (many cells): every point has its twin
    and the four points of the two adjacent nodes within eps -- six with itself, core at min_samples = 5 -- and nothing else."""
    t = np.arange(nodes, dtype=np.float64) * step
    u = np.array([0.8, 0.5, np.sqrt(1 - 0.8 ** 2 - 0.5 ** 2)])
    node = np.array([-400.0, 30.0, -60.0]) + t[:, None] * u[None, :]
    return np.repeat(node, 2, 0).astype(F32)


def _mixture(seed, B=None, C=None):
    """Up to 2,000 points in 1-3 scans and 1-3 classes: Gaussian blobs of unequal density, uniform clutter, in every third case
    snapped to a 1 m lattice (exact ties and duplicates)."""
    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    B, C = B or 1 + seed % 3, C or 1 + (seed // 3) % 3
    class_ids = [3, 11, 250][:C]
    sets, labs = [], []
    for b in range(B):
        parts, lab = [], []
        for k in range(int(rng.integers(2, 8))):
            r = rng.choice([4.0, 9.0, 25.0, 40.0]) + rng.uniform(-1, 1)
            a = rng.uniform(0, 2 * np.pi)
            n = int(rng.integers(3, 70))
            parts.append(_blob(rng, n, (r * np.cos(a), r * np.sin(a), rng.uniform(-2, 1)), rng.choice([0.3, 1.0, 2.5])))
            lab.append(np.full(n, rng.choice(class_ids + [0])))
        n = int(rng.integers(20, 150))
        parts.append(rng.uniform(-45, 45, (n, 3)).astype(F32) * np.array([1, 1, 0.1], F32))
        lab.append(rng.choice(class_ids + [0], n))
        P, L = np.concatenate(parts), np.concatenate(lab)
        if seed % 3 == 2:
            P = np.round(P)
        perm = rng.permutation(len(P))
        sets.append(np.ascontiguousarray(P[perm], F32))
        labs.append(L[perm].astype(np.int64))
    assert sum(len(p) for p in sets) <= 2000
    return dict(points=sets, labels=labs, class_ids=class_ids)


def build_cases():
    """name -> dict(points=[(N_b, cols) float32], labels=[(N_b,) int], class_ids=[...], and optionally eps / min_samples /
    max_distance / include_noise)."""
    rng = np.random.Generator(np.random.PCG64(2025))
    one = lambda P, L=None, ids=(1,), **kw: dict(points=[np.ascontiguousarray(P, F32)],                     # noqa: E731
                                                 labels=[np.full(len(P), ids[0], np.int64) if L is None else np.asarray(L)],
                                                 class_ids=list(ids), **kw)
    c = {}
    c["empty scan"] = one(np.zeros((0, 3), F32))
    c["no point of a requested class"] = one(_blob(rng, 100, (5, 0, 0), 1.0), np.zeros(100, np.int64), ids=(1, 2))
    c["one point"] = one([[3.0, 4.0, -1.0]])
    c["four points"] = one(_blob(rng, 4, (6, 2, -1), 0.2))
    c["five coincident points"] = one(np.tile([[7.0, -3.0, 0.5]], (5, 1)))
    # five within eps of each other next to four: a cluster and noise
    c["min_samples and one fewer"] = one(np.concatenate([_blob(rng, 5, (8, 0, 0), 0.3), _blob(rng, 4, (-8, 30, 0), 0.3)]))
    # a 3 x 3 x 3 lattice of side 4 (the face neighbours at exactly eps): centre and face centres are core (7 and 6), edges (5) too,
    # corners (4) are border points; three classes: the same with side nextafter(4) (nobody has a neighbour), and pairs of triple
    # points exactly 4 (one cluster of 6) and nextafter(4) (noise) apart
    g = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    up = np.nextafter(F32(4.0), F32(5.0))
    lat = np.concatenate([g * 4.0, g * np.float64(up), np.repeat([[0, 0, 8.0], [4.0, 0, 8.0]], 3, 0) + [0, 40, 0],
                          np.repeat([[0, 0, 8.0], [up, 0, 8.0]], 3, 0) + [0, 40, 0]]).astype(F32)
    c["ties at eps on a lattice"] = one(lat, np.concatenate([np.full(27, 1), np.full(27, 2), np.full(6, 3), np.full(6, 4)]), ids=(1, 2, 3, 4))
    ch = _chain(rng)
    blob2 = _blob(rng, 40, (0, 5, 0), 0.5)
    c["chain, lowest core at the near end"] = one(np.concatenate([ch, blob2]))
    mid = np.concatenate([ch[300:], ch[:300]])
    c["chain, lowest core in the middle"] = one(np.concatenate([mid[:20], blob2, mid[20:]]))
    c["chain, lowest core at the far end"] = one(np.concatenate([blob2[:7], ch[::-1], blob2[7:]]))
    c["chain, shuffled"] = one(np.concatenate([ch, blob2])[rng.permutation(640)])
    # a0 with four mates 3 m behind it, b0 likewise, 7.8 m apart; the bridge at 3.9 m from both sees a0, b0 and itself: not core
    mates = lambda x: np.array([[x, 0.1 * k, 0] for k in range(4)])                                        # noqa: E731
    A, Bc = np.concatenate([[[0, 0, 0]], mates(-3.0)]), np.concatenate([[[7.8, 0, 0]], mates(10.8)])
    bridge = np.array([[3.9, 0, 0]])
    c["a border point between two clusters, last"] = one(np.concatenate([Bc, A, bridge]))
    c["a border point between two clusters, first"] = one(np.concatenate([bridge, A, Bc]))
    # row 0 is a border point of X; Y's core points come before X's: Y is cluster 0, X cluster 1, row 0 gets 1
    X = np.concatenate([[[50, 0, 0]], mates(47.0)])
    c["lowest index is a border point"] = one(np.concatenate([[[53.9, 0, 0]], A, X]))
    # cells: negative coordinates, points on cell boundaries (multiples of eps), +-200 m
    edge = np.array([[x, y, z] for x in (-8.0, -4.0, 0.0, 4.0) for y in (-4.0, 0.0) for z in (-4.0, 0.0, 4.0)])
    far = np.concatenate([_blob(rng, 60, (-200, 199.5, -3), 1.5), _blob(rng, 60, (200.5, -200, 2), 1.5), _blob(rng, 30, (-196.1, -203.9, 0), 2.0)])
    c["cell boundaries"] = one(np.concatenate([edge, edge + [-0.0, 0, 0], far, np.nextafter(edge.astype(F32), F32(-1e9))]), max_distance=250.0)
    c["a blob inside one cell"] = one(rng.uniform(0.1, 3.9, (3000, 3)))
    # three coincident points per (scan, class): noise when isolated, a cluster of six if two segments were merged; five: a cluster each
    tri = np.concatenate([np.tile([[5.0, 5, 0]], (3, 1)), np.tile([[-9.0, 2, 0]], (5, 1))])
    two = dict(points=[np.concatenate([tri, tri]).astype(F32)] * 2, labels=[np.repeat([1, 2], 8).astype(np.int64)] * 2, class_ids=[1, 2])
    c["the same points in two scans and two classes"] = two
    m = _mixture(100, B=3, C=3)
    sets, labs = m["points"], m["labels"]
    labs[1] = np.where(labs[1] == 11, 0, labs[1])          # scan 1 has no class 11; nobody has class 99
    c["three scans, three classes, an empty segment"] = dict(points=sets, labels=labs, class_ids=[3, 11, 99])
    noisy = np.concatenate([_blob(rng, 50, (5, 1, 0), 0.8), _blob(rng, 50, (-30, 5, 0), 0.8), rng.uniform(-12, 12, (12, 3)) * [1, 1, 0.05] + [0, 60, 0],
                            [[2.0, 9.0, 0]]])
    c["noise group kept"] = one(noisy)
    c["noise group dropped"] = one(noisy, include_noise=False)
    bad = np.concatenate([_blob(rng, 40, (6, 0, 0), 0.7), _blob(rng, 30, (0, -9, 0), 0.7)]).astype(F32)
    L = np.ones(70, np.int64)
    bad[3, 0] = np.nan
    bad[11, 1] = np.inf
    bad[12, 2] = -np.inf
    bad[40, 2] = np.nan
    bad[50] = [4.0 * 2 ** 20, 0, 0]                       # |x| / eps = 2^20: out of the grid
    bad[51] = [0, -(4.0 * 2 ** 20 - 4), 0]                # the last cell inside it: a noise point
    bad[60, 0] = np.nan
    L[60] = 0                                            # not of a requested class: not counted
    c["rejected rows"] = one(bad, L, max_distance=1e7)
    # uint8 / int32 labels, a fourth column carried through, other parameters
    m1, m2 = _mixture(101, B=1, C=3), _mixture(102, B=2, C=2)
    wide = np.concatenate([m1["points"][0], rng.random((len(m1["points"][0]), 2), dtype=F32)], 1)
    c["five columns, uint8 labels, eps 1.5"] = dict(points=[wide], labels=[m1["labels"][0].astype(np.uint8)], class_ids=[3, 11, 250], eps=1.5,
                                                   min_samples=3, max_distance=20.0)
    c["int32 labels, negative class id"] = dict(points=m2["points"], labels=[np.where(x == 3, -7, x).astype(np.int32) for x in m2["labels"]],
                                                class_ids=[-7, 11])
    for k in range(20):
        c[f"mixture {k}"] = _mixture(k)
    return c


def params_of(case):
    return {k: case[k] for k in ("eps", "min_samples", "max_distance", "include_noise") if k in case}


def segments(case):
    """The accepted points of every (scan, class) of a case, in row order."""
    eps = case.get("eps", EPS)
    for P, L in zip(case["points"], case["labels"]):
        ok = accepted(P, eps)
        for cid in case["class_ids"]:
            yield np.asarray(P, F32)[(np.asarray(L).astype(np.int64) == cid) & ok][:, :3]
