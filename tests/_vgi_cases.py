"""Inputs and numpy references of the VGI edge tests (tests/test_gpu_vgi_edges.py runs them on the device,
tests/test_vgi_cases_host.py checks that every input holds the edge it is named after and that the references agree with
oracle/vgi.py wherever that has the function).  No GPU, no torch.

One restatement per entry point of csrc/vgi.hip, written from the contract in that file's comments.  Every coordinate is a
multiple of 2^-10, projection matrices hold small integers and powers of two, centres are multiples of 0.25: float32 and float64
sums are exact in any order, so every comparison is an equality.  Grids are small (X, Y <= 20 cells; the z volume keeps the
library's 128 slots), clouds hold 1 .. 3000 points, range images are 16x4 and 64x8.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle import vgi as ovgi

INT_MAX = 2 ** 31 - 1
ZR = 128                 # z slots of the map (csrc/vgi.hip: VGI_ZR)
ZLO = -ZR // 2           # mopa_amd/vgi.py: zlo
Q = 1024.0               # coordinates are multiples of 1 / Q
E = 1.0 / Q


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ------------------------------------------------------------------------------------------------ the search map
MAPS = {"vs0.5_x": (0.5, (4.0, 4.0), "x"), "vs0.5_y": (0.5, (4.0, 4.0), "y"), "vs0.25_x": (0.25, (2.5, 2.5), "x"),
        "vs0.25_y": (0.25, (2.5, 2.5), "y"), "vs1_x": (1.0, (4.0, 4.0), "x"), "vs1_y": (1.0, (4.0, 4.0), "y"),
        "vs0.5_x_rect": (0.5, (4.0, 2.5), "x")}


def map_geometry(vs, search_range, front):
    """OverlapMap's numbers: origin cell (ox, oy) in voxel units, size X x Y cells."""
    sr = [int(search_range[0] / vs), int(search_range[1] / vs)]
    ox, oy = (0, -sr[1]) if front == "x" else (-sr[0], 0)
    return dict(vs=vs, ox=ox, oy=oy, X=2 * sr[0], Y=2 * sr[1], zlo=ZLO, front=front, search_range=search_range)


def voxel_f32(pts, vs):
    """floor(p / voxel_size) with a float32 quotient, like numpy's `pc[:, :3] / voxel_size` on a float32 cloud."""
    assert pts.dtype == np.float32
    return np.floor(pts[:, :3] / np.float32(vs)).astype(np.int64)


def voxel_f64(pts, vs):
    """sparse_quantize's voxel: floor of the float64 quotient."""
    return np.floor(pts[:, :3].astype(np.float64) / vs).astype(np.int64)


def pad_stride(pts, stride):
    """(n, 3) -> (n, stride): further columns hold values that would show as wrong voxels if they were read as coordinates."""
    out = np.full((len(pts), stride), 777.0, np.float32)
    out[:, :3] = pts
    return out


# ------------------------------------------------------------------------------------------------ mopa_vgi_first_points
def ref_first_points(pts, vs, ox, oy, X, Y, zlo, g_mask=None):
    """-> (first (X*Y*ZR,) int32, status): first[(cx * Y + cy) * ZR + cz] = smallest index of the points of that voxel, INT_MAX if
    none; status bit 0 = a point with a ground flag lies inside the map in x / y and outside its z slots."""
    c = voxel_f32(pts, vs) - np.array([ox, oy, zlo])
    inxy = (c[:, 0] >= 0) & (c[:, 0] < X) & (c[:, 1] >= 0) & (c[:, 1] < Y)
    inz = (c[:, 2] >= 0) & (c[:, 2] < ZR)
    first = np.full(X * Y * ZR, INT_MAX, np.int32)
    idx = np.nonzero(inxy & inz)[0]
    np.minimum.at(first, (c[idx, 0] * Y + c[idx, 1]) * ZR + c[idx, 2], idx.astype(np.int32))
    status = 0 if g_mask is None else int(bool((np.asarray(g_mask, bool) & inxy & ~inz).any()))
    return first, status


def ref_first_points_rep(pts, vs, ox, oy, X, Y, zlo):
    """mopa_vgi_first_points_rep: only the first point of every FLOAT64 voxel marks, at the cell of its FLOAT32 floor."""
    _, rep = np.unique(voxel_f64(pts, vs), axis=0, return_index=True)
    rep = np.sort(rep)
    first, _ = ref_first_points(pts[rep], vs, ox, oy, X, Y, zlo)
    hit = first != INT_MAX
    first[hit] = rep[first[hit]].astype(np.int32)
    return first


FIRST_SIZES = [1, 63, 64, 65, 3000]


def first_cloud(vs, search_range, front, n=3000, seed=0):
    """-> (pts (n, 3) float32, names {edge name: row}).  The edge rows come first (a prefix of 63 rows holds them all), random
    rows over the map and one cell around it follow; the last row repeats the duplicated point."""
    g = map_geometry(vs, search_range, front)
    F, L = (g["X"], g["Y"]) if front == "x" else (g["Y"], g["X"])     # forward axis: cells 0 .. F-1, lateral: -L/2 .. L/2-1
    rows, names = [], {}

    def add(name, fwd, lat, z):
        """Coordinates in metres; `fwd` / `lat` = along / across the front axis."""
        names[name] = len(rows)
        rows.append((fwd, lat, z) if front == "x" else (lat, fwd, z))

    in_f, in_l, in_z = 2.5 * vs, 1.5 * vs, 0.5 * vs
    add("neg_face", in_f, -vs, -vs)                                  # -vs / vs = -1 exactly: voxel -1, not 0
    add("dup_a", in_f + vs, in_l, in_z)
    add("dup_b", in_f + vs, in_l, in_z)
    add("f_first", 0.0, in_l, in_z)                                  # on the face of the first cell
    add("f_below", -E, in_l, in_z)                                   # just outside
    add("f_last", F * vs - E, in_l, in_z)                            # last cell
    add("f_out", F * vs, in_l, in_z)                                 # on the outer face of the last cell: outside
    add("l_first", in_f, -L / 2 * vs, in_z)
    add("l_below", in_f, -L / 2 * vs - E, in_z)
    add("l_last", in_f, L / 2 * vs - E, in_z)
    add("l_out", in_f, L / 2 * vs, in_z)
    add("z_slot0", in_f + 2 * vs, in_l, ZLO * vs)
    add("z_below", in_f + 2 * vs, in_l, ZLO * vs - E)                # slot -1: dropped
    add("z_slot127", in_f + 2 * vs, in_l, (ZLO + ZR) * vs - E)
    add("z_slot128", in_f + 2 * vs, in_l, (ZLO + ZR) * vs)           # dropped
    add("xy_out_z_out", -2 * vs, in_l, ZLO * vs - E)                 # outside in x / y AND in z: not a dropped point of the map
    rng = _rng(seed)
    m = max(n - len(rows), 0)
    fwd = rng.integers(int(-vs * Q), int((F + 1) * vs * Q), m) / Q
    lat = rng.integers(int((-L / 2 - 1) * vs * Q), int((L / 2 + 1) * vs * Q), m) / Q
    z = rng.integers(int(-6 * vs * Q), int(6 * vs * Q), m) / Q
    fill = np.stack([fwd, lat, z] if front == "x" else [lat, fwd, z], 1)
    pts = np.concatenate([np.asarray(rows, np.float64).reshape(-1, 3), fill], 0)[:n].astype(np.float32)
    if n > len(rows) + 1:
        pts[-1] = pts[names["dup_a"]]
        names["dup_last"] = n - 1
    return pts, {k: v for k, v in names.items() if v < n}


def first_masks(pts, vs, g, seed=1):
    """Ground flags for a first_cloud: `ground_dropped` flags a point that the z slots drop (status 1), `nonground_dropped` flags
    none of them -- but the point that is outside in x / y too (status 0)."""
    c = voxel_f32(pts, vs) - np.array([g["ox"], g["oy"], g["zlo"]])
    inxy = (c[:, 0] >= 0) & (c[:, 0] < g["X"]) & (c[:, 1] >= 0) & (c[:, 1] < g["Y"])
    dropped = inxy & ((c[:, 2] < 0) | (c[:, 2] >= ZR))
    base = _rng(seed).integers(0, 2, len(pts)).astype(np.uint8)
    base[dropped] = 0
    a, b = base.copy(), base.copy()
    if dropped.any():
        a[np.nonzero(dropped)[0][-1]] = 1
    b[~inxy & ((c[:, 2] < 0) | (c[:, 2] >= ZR))] = 1
    return {"ground_dropped": a, "nonground_dropped": b}, dropped


# ------------------------------------------------------------------------------------------------ mopa_vgi_box_free
BOX_X, BOX_Y = 16, 10


def ref_box_free(first, X, Y, zlo, gz0, Z, bx, by, bz):
    """free[Xo][Yo][Zo] = 1 where the bx x by x bz box at that cell meets no occupied voxel of the slab [gz0, gz0 + Z)."""
    z0 = gz0 - zlo
    occ = (first.reshape(X, Y, ZR) != INT_MAX)[:, :, z0:z0 + Z]
    return (~sliding_window_view(occ, (bx, by, bz)).any(axis=(3, 4, 5))).astype(np.uint8)


def _first_of(occ, seed=0):
    """A `first` volume with the given occupancy: occupied voxels hold point indices (0 included)."""
    idx = _rng(seed).integers(0, 3000, occ.shape).astype(np.int32)
    idx.reshape(-1)[np.argmax(occ.reshape(-1))] = 0
    return np.where(occ, idx, INT_MAX).astype(np.int32).reshape(-1)


def box_cases():
    """name -> dict(first, X, Y, zlo, gz0, Z, box).  Outside the slab the volume is randomly occupied in every case."""
    X, Y = BOX_X, BOX_Y
    rng = _rng(11)

    def vol(p_in, gz0, Z, p_out=0.5):
        occ = rng.random((X, Y, ZR)) < p_out
        z0 = gz0 - ZLO
        occ[:, :, z0:z0 + Z] = rng.random((X, Y, Z)) < p_in
        return occ

    def case(occ, gz0, Z, box):
        return dict(first=_first_of(occ), X=X, Y=Y, zlo=ZLO, gz0=gz0, Z=Z, box=box)

    c = {}
    c["box_1x1x1"] = case(vol(0.3, -4, 8), -4, 8, (1, 1, 1))
    c["bx_eq_X"] = case(vol(0.01, -4, 8), -4, 8, (X, 3, 2))
    c["bx_by_eq_XY"] = case(vol(0.003, -4, 8), -4, 8, (X, Y, 2))
    c["box_eq_grid_free"] = case(vol(0.0, -4, 8), -4, 8, (X, Y, 8))
    occ = vol(0.0, -4, 8)
    occ[X - 1, Y - 1, 60 + 7] = True
    c["box_eq_grid_taken"] = case(occ, -4, 8, (X, Y, 8))
    c["bz_eq_Z"] = case(vol(0.02, -4, 8), -4, 8, (3, 3, 8))
    c["empty_grid"] = case(vol(0.0, -4, 8), -4, 8, (3, 2, 2))
    occ = vol(0.0, -4, 8)
    occ[5, 4, 60:68] = True
    c["full_column"] = case(occ, -4, 8, (2, 3, 2))
    occ = vol(0.0, -4, 8, p_out=0.0)
    for x in (0, X - 1):
        for y in (0, Y - 1):
            occ[x, y, 60] = occ[x, y, 67] = True
    occ[:, :, 59] = occ[:, :, 68] = True            # the slots next to the slab are full: they must not count
    c["eight_corners"] = case(occ, -4, 8, (2, 2, 2))
    c["slab_at_slot_0"] = case(vol(0.1, ZLO, 8), ZLO, 8, (3, 4, 2))
    c["slab_to_slot_128"] = case(vol(0.1, ZLO + ZR - 8, 8), ZLO + ZR - 8, 8, (3, 4, 2))
    c["whole_volume"] = case(vol(0.02, ZLO, ZR), ZLO, ZR, (2, 2, 5))
    c["sparse"] = case(vol(0.05, -4, 9), -4, 9, (3, 4, 2))
    return c


# (X, Y, gz0, Z, bx, by, bz): every one is refused
BOX_REFUSED = {"bx_gt_X": (16, 10, -4, 8, 17, 1, 1), "by_gt_Y": (16, 10, -4, 8, 1, 11, 1), "bz_gt_Z": (16, 10, -4, 8, 1, 1, 9),
               "z0_negative": (16, 10, ZLO - 1, 8, 1, 1, 1), "slab_past_128": (16, 10, ZLO + ZR - 7, 8, 1, 1, 1),
               "X_0": (0, 10, -4, 8, 1, 1, 1), "Y_neg": (16, -1, -4, 8, 1, 1, 1), "Z_0": (16, 10, -4, 0, 1, 1, 1),
               "bx_0": (16, 10, -4, 8, 0, 1, 1), "by_neg": (16, 10, -4, 8, 1, -2, 1), "bz_0": (16, 10, -4, 8, 1, 1, 0)}


# ------------------------------------------------------------------------------------------------ ground columns, road height
def ref_ground_cells(first, g_mask, X, Y):
    """ground2d[cx * Y + cy] = 1 iff some voxel of the column has a FIRST point with a ground flag."""
    f = first.reshape(X * Y, ZR)
    occ = f != INT_MAX
    flag = np.zeros(f.shape, bool)
    flag[occ] = np.asarray(g_mask, bool)[f[occ]]
    return flag.any(1).astype(np.uint8)


def ref_road_height(pts, vs, first, g_mask, ox, oy, X, Y, zlo, cell):
    """(sum of z, count) over ALL points (ground or not) of the lowest voxel of column `cell` whose first point is ground;
    (0, 0) when the column has none."""
    f = first.reshape(X, Y, ZR)[cell[0] - ox, cell[1] - oy]
    g = np.asarray(g_mask, bool)
    slots = [z for z in range(ZR) if f[z] != INT_MAX and g[f[z]]]
    if not slots:
        return 0.0, 0.0
    v = voxel_f32(pts, vs)
    m = (v[:, 0] == cell[0]) & (v[:, 1] == cell[1]) & (v[:, 2] == zlo + slots[0])
    return float(pts[m, 2].astype(np.float64).sum()), float(m.sum())


ROAD_SIZES = [1, 1023, 1025, 3000]
GROUND_CELLS = dict(top=(2, -3), mixed=(3, -3), late=(4, -3), early=(5, -3), two=(6, -3))    # columns in voxel units, front x


def ground_cloud(n=3000, seed=0):
    """-> (pts (n, 3) float32, g_mask (n,) uint8, g = map_geometry(0.5, (4, 4), "x")).  Five columns hold one edge each (rows
    first), random points with random flags fill the other columns; a third of the rows behind them fall into the lowest voxel
    of column `two`, ground and not, spread over every index range.
      top:   its only ground voxel is z slot 127; lower voxels are not ground
      mixed: ground and non-ground voxels
      late:  one voxel whose first point is not ground and whose second is -> by the first-point rule the column is NOT ground
      early: one voxel whose first point is ground and whose second is not -> ground
      two:   ground voxels at z voxels -3 and 1; the lower one is shared with non-ground points, which count for the height"""
    vs = 0.5
    g = map_geometry(vs, (4.0, 4.0), "x")
    rows, flags = [], []

    def add(cell, vz, ground, dx=0.25, dy=0.25, dz=0.25):
        rows.append(((cell[0]) * vs + dx, (cell[1]) * vs + dy, vz * vs + dz))
        flags.append(ground)

    C = GROUND_CELLS
    add(C["two"], -3, 1, dz=0.125)                  # row 0: the n = 1 cloud is this point
    add(C["two"], -3, 0, dz=0.375)
    add(C["two"], 1, 1)
    add(C["two"], 0, 0)
    add(C["top"], ZLO + ZR - 1, 1)
    add(C["top"], -2, 0)
    add(C["top"], 5, 0)
    add(C["mixed"], -4, 0)
    add(C["mixed"], -2, 1)
    add(C["mixed"], 3, 0)
    add(C["late"], -1, 0)
    add(C["late"], -1, 1, dz=0.375)
    add(C["early"], -1, 1)
    add(C["early"], -1, 0, dz=0.375)
    rng = _rng(seed)
    m = max(n - len(rows), 0)
    x = rng.integers(0, int(8 * Q), m) / Q
    y = rng.integers(int(-4 * Q), int(4 * Q), m) / Q
    z = rng.integers(int(-3 * Q), int(3 * Q), m) / Q
    y[(y >= -1.5) & (y < -1.0)] += 1.0              # keep the filler out of row y = -3 (the five columns)
    fill, ff = np.stack([x, y, z], 1), rng.integers(0, 2, m)
    third = rng.random(m) < 1 / 3
    k = int(third.sum())
    fill[third] = np.stack([C["two"][0] * vs + rng.integers(0, 512, k) / Q, C["two"][1] * vs + rng.integers(0, 512, k) / Q,
                            -3 * vs + rng.integers(0, 512, k) / Q], 1)
    pts = np.concatenate([np.asarray(rows, np.float64), fill], 0)[:n].astype(np.float32)
    return pts, np.concatenate([flags, ff])[:n].astype(np.uint8), g


# ------------------------------------------------------------------------------------------------ mopa_vgi_candidates
def ref_candidates(free, ext, off, vs, ori_range, P, image_size, g2d, ox, oy, X, Y):
    """-> (cand2d (X*Y,) uint8, (n_free, n_kept)): a free cell's centre (start + (extent - 1) / 2 + offset) * voxel_size, float64,
    passes when x > 0, its float32 projection lies strictly inside the image and its range is >= ori_range; the (x, y) cell of
    a passing centre is marked when it is inside the map and a ground column."""
    idx = np.argwhere(free)
    c = (idx + (np.asarray(ext, np.float64) - 1) / 2 + np.asarray(off, np.float64)) * vs
    m = c[:, 0] > 0
    h, P32 = c.astype(np.float32), np.asarray(P, np.float64).astype(np.float32)
    p = [((P32[r, 0] * h[:, 0] + P32[r, 1] * h[:, 1]) + P32[r, 2] * h[:, 2]) + P32[r, 3] for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = p[0] / p[2], p[1] / p[2]
    m &= (u > 0) & (v > 0) & (u < np.float32(image_size[0])) & (v < np.float32(image_size[1]))
    m &= np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) >= ori_range
    cand = np.zeros(X * Y, np.uint8)
    f = np.floor(c[m][:, :2] / vs).astype(np.int64) - np.array([ox, oy])
    f = f[(f[:, 0] >= 0) & (f[:, 0] < X) & (f[:, 1] >= 0) & (f[:, 1] < Y)]
    at = f[:, 0] * Y + f[:, 1]
    cand[at[g2d[at] != 0]] = 1
    return cand, (len(idx), int(m.sum()))


def cand_centres(case):
    """The centres of a case's free cells in metres (float64), in row-major order -- `check_overlap`'s return value."""
    return (np.argwhere(case["free"]) + (case["ext"] - 1) / 2 + case["off"]) * case["vs"]


def cand_projection(case, centres):
    """float32 (u, v, p2) of centres, with the oracle's own matmul."""
    h = np.concatenate((centres, np.ones((len(centres), 1))), axis=1)
    p = np.matmul(case["P"].astype(np.float32), h.astype(np.float32).T, dtype=np.float32).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], p[:, 2]


def ori_range_of(obj):
    oc = (np.max(obj, axis=0) + np.min(obj, axis=0)) / 2
    return float(np.sqrt(np.square(oc[0]) + np.square(oc[1])))


def oracle_candidates(case):
    """The same through oracle/vgi.py: filter_centers + ground_centers on the case's scan -> (cand2d, (n_free, n_kept))."""
    g = case["g"]
    vc0 = cand_centres(case)
    vc = ovgi.filter_centers(vc0, case["obj"], case["P"], case["image_size"])
    cand = np.zeros(g["X"] * g["Y"], np.uint8)
    cells = ovgi.ground_centers(case["scan"], vc, case["g_mask"], case["vs"])[0] if len(vc) else None
    if cells is not None:
        f = cells.astype(np.int64) - np.array([g["ox"], g["oy"]])
        cand[f[:, 0] * g["Y"] + f[:, 1]] = 1
    return cand, (len(vc0), len(vc))


def _floor_scan(g, holes=(), seed=0):
    """One ground point per column of the map at z voxel -4 (0.25 inside its voxel); in the `holes` the first point of that
    voxel is not ground (a ground point follows it: still not a ground column)."""
    vs = g["vs"]
    cx, cy = np.meshgrid(np.arange(g["X"]) + g["ox"], np.arange(g["Y"]) + g["oy"], indexing="ij")
    cells = np.stack([cx.reshape(-1), cy.reshape(-1)], 1)
    cells = cells[_rng(seed).permutation(len(cells))]
    pts = np.concatenate([cells * vs + vs / 2, np.full((len(cells), 1), -4 * vs + vs / 2)], 1)
    flags = np.ones(len(cells), np.uint8)
    hole = np.array([tuple(c) in set(holes) for c in cells.tolist()], bool)
    flags[hole] = 0
    pts = np.concatenate([pts, pts[hole]], 0)
    flags = np.concatenate([flags, np.ones(int(hole.sum()), np.uint8)])
    return pts.astype(np.float32), flags


def cand_cases():
    """name -> dict(g, vs, free, ext, off, obj, ori_range, P, image_size, scan, g_mask).  Front x: u = 2 - 2 cy / cx, v = 1 - 2 cz / cx
    in a 4 x 2 image, so u == 0 on cy == cx, u == img_w on cy == -cx, v == 0 on cz == cx / 2, v == img_h on cz == -cx / 2, all
    exact; extent (1, 1, 1) puts cx == 0 on the first row of cells.  behind_camera_x: p2 = cx - cy + 1/8 is negative for cy > cx, and
    with p0, p1 < 0 everywhere exactly those centres project into the image -- the reference has no test of the sign of p2.  Front y likewise with the axes swapped (extent (1, 3, 1):
    cy >= 0.5, no division by zero)."""
    out = {}

    def case(name, front, free, ext, obj, P, image_size, vs=0.5, sr=(4.0, 4.0), holes=()):
        g = map_geometry(vs, sr, front)
        scan, flags = _floor_scan(g, holes)
        obj = np.asarray(obj, np.float64)
        out[name] = dict(g=g, vs=vs, free=np.ascontiguousarray(free, np.uint8), ext=np.asarray(ext, np.float64),
                         off=np.array([g["ox"], g["oy"], np.floor(-2.0 / vs)], np.float64), obj=obj, ori_range=ori_range_of(obj),
                         P=np.asarray(P, np.float64), image_size=image_size, scan=scan, g_mask=flags)

    Px = [[2, -2, 0, 0], [1, 0, -2, 0], [1, 0, 0, 0]]
    Py = [[2, 2, 0, 0], [0, 1, -2, 0], [0, 1, 0, 0]]
    centred = [[-1, -1, 0], [1, 1, 0]]                          # ori_range 0
    ones = np.ones((16, 16, 10), np.uint8)
    case("image_bounds_x", "x", ones, (1, 1, 1), centred, Px, (4, 2))
    case("image_bounds_y", "y", ones[:, :14], (1, 3, 1), centred, Py, (4, 2))
    case("range_345_x", "x", ones, (1, 1, 1), [[1.5, 1.0, 0], [2.5, 2.0, 0]], Px, (4, 2))          # centre (2, 1.5): range 2.5
    case("range_345_y", "y", ones[:, :14], (1, 3, 1), [[1.0, 1.5, 0], [2.0, 2.5, 0]], Py, (4, 2))  # centre (1.5, 2)
    case("behind_camera_x", "x", ones, (1, 1, 1), centred, [[1, -1, 0, -8], [0, 0, -1, -8], [1, -1, 0, 0.125]], (128, 128))
    wide = [[64, -1, 0, 0], [64, 0, -1, 0], [1, 0, 0, 0]]
    case("every_cell_passes", "x", np.ones((15, 15, 9), np.uint8), (2, 2, 2), centred, wide, (128, 128))
    case("no_free_cell", "x", np.zeros((15, 15, 9), np.uint8), (2, 2, 2), centred, wide, (128, 128))
    case("cells_not_ground", "x", np.ones((15, 15, 9), np.uint8), (2, 2, 2), centred, wide, (128, 128),
         holes=[(0, -8), (3, 2), (7, -1), (14, 6)])
    rng = _rng(5)
    case("random_free_x", "x", rng.random((14, 13, 7)) < 0.3, (3, 4, 2), [[1.0, 0.5, 0], [2.0, 1.0, 0]], Px, (4, 2), holes=[(4, -1), (5, -2)])
    case("random_free_y_quarter", "y", rng.random((18, 18, 5)) < 0.3, (3, 3, 1), [[0.25, 0.5, 0], [0.75, 1.0, 0]], Py, (4, 2), vs=0.25,
         sr=(2.5, 2.5), holes=[(1, 9), (4, 15)])
    return out


# ------------------------------------------------------------------------------------------------ mopa_vgi_compact_cells
COMPACT_MAPS = [(1, 1), (33, 31), (32, 32), (25, 41), (3, 683)]          # 1, 1023, 1024, 1025, 2049 cells
COMPACT_FILLS = ["none", "all", "last", "every65"]


def compact_input(X, Y, fill):
    c = np.zeros(X * Y, np.uint8)
    if fill == "all":
        c[:] = 1
    elif fill == "last":
        c[-1] = 1
    elif fill == "every65":
        c[::65] = 1
    return c


def ref_compact(cand2d, X, Y, ox, oy):
    """-> (cells (m, 2) int32 in voxel units, m): the marked cells in row-major order."""
    cells = np.argwhere(cand2d.reshape(X, Y) != 0) + np.array([ox, oy])
    return cells.astype(np.int32), len(cells)


# ------------------------------------------------------------------------------------------------ mopa_vgi_range_keep
def range_real_pixels(pts, fov_up, fov_down, W, H):
    """The real-valued (column, row) before floor and clamp, and the depth."""
    fov = abs(fov_down) + abs(fov_up)
    depth = np.sqrt(pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1] + pts[:, 2] * pts[:, 2])
    px = 0.5 * (-np.arctan2(pts[:, 1], pts[:, 0]) / np.pi + 1.0) * W
    py = (1.0 - (np.arcsin(pts[:, 2] / depth) + abs(fov_down)) / fov) * H
    return px, py, depth


def ref_range_keep(pts, n_scan, fov_up, fov_down, W, H):
    """keep[i] = 0 iff i's pixel holds an object point (rows from n_scan on) and i is not that pixel's nearest point (ties: the
    smaller index)."""
    px, py, depth = range_real_pixels(pts, fov_up, fov_down, W, H)
    col = np.clip(np.floor(px), 0, W - 1).astype(np.int64)
    row = np.clip(np.floor(py), 0, H - 1).astype(np.int64)
    pix = row * W + col
    keep = np.ones(len(pts), bool)
    for q in np.unique(pix[n_scan:]):
        members = np.nonzero(pix == q)[0]
        keep[members] = False
        keep[members[np.argmin(depth[members])]] = True       # argmin: the first of equal depths = the smaller index
    return keep


def range_point(col, row, depth, W, H, fov_up, fov_down, pitch=None):
    """The point of the given depth at the CENTRE of pixel (col, row), rounded to multiples of 2^-10 (pixels are >= 0.1 rad wide)."""
    fov = abs(fov_down) + abs(fov_up)
    yaw = ((col + 0.5) / W * 2.0 - 1.0) * np.pi
    if pitch is None:
        pitch = (1.0 - (row + 0.5) / H) * fov - abs(fov_down)
    p = depth * np.array([np.cos(pitch) * np.cos(-yaw), np.cos(pitch) * np.sin(-yaw), np.sin(pitch)])
    return np.round(p * Q) / Q


FOV = (0.05235, -0.43633)          # the library's defaults
FOV_EXACT = (0.25, -0.75)          # fov = 1: a point with z = 0 lies exactly on the face between rows H/4 - 1 and H/4


def range_cases():
    """name -> dict(pts (n, 3) float64, n_scan, W, H, fov_up, fov_down, expect {row: kept?} for the rows the case is about)."""
    out = {}

    def case(name, scan, obj, W, H, expect=None, fov=FOV, **kw):
        pts = np.asarray(list(scan) + list(obj), np.float64).reshape(-1, 3)
        out[name] = dict(pts=pts, n_scan=len(scan), W=W, H=H, fov_up=fov[0], fov_down=fov[1], expect=expect or {}, **kw)

    def P(col, row, d, W=16, H=4, **kw):
        return range_point(col, row, d, W, H, *FOV, **kw)

    a, b, c = P(3, 1, 4.0), P(9, 2, 5.0), P(12, 0, 3.0)
    case("tie2_scan_and_object", [a, P(3, 1, 6.0)], [a], 16, 4, {0: True, 1: False, 2: False}, ties=[(0, 2)])
    case("tie2_two_objects", [P(9, 2, 7.0)], [b, b], 16, 4, {0: False, 1: True, 2: False}, ties=[(1, 2)])
    case("tie3_scan_scan_object", [c, c, P(12, 0, 3.5)], [c, P(12, 0, 6.0)], 16, 4, {0: True, 1: False, 2: False, 3: False, 4: False},
         ties=[(0, 1), (1, 3)])
    case("tie3_three_objects", [], [c, c, c], 16, 4, {0: True, 1: False, 2: False}, ties=[(0, 1), (1, 2)])
    case("scan_only_pixel_keeps_all", [P(5, 3, 3.0), P(5, 3, 4.0), P(5, 3, 5.0), a], [P(3, 1, 3.0)], 16, 4,
         {0: True, 1: True, 2: True, 3: False, 4: True})
    case("scan_in_front_of_objects", [P(7, 2, 3.0)], [P(7, 2, 5.0), P(7, 2, 6.0)], 16, 4, {0: True, 1: False, 2: False})
    case("object_in_front_of_scan", [P(7, 2, 5.0), P(7, 2, 6.0)], [P(7, 2, 3.0)], 16, 4, {0: False, 1: False, 2: True})
    case("all_object_points", [], [a, P(3, 1, 6.0), b], 16, 4, {0: True, 1: False, 2: True})
    case("all_scan_points", [a, a, P(3, 1, 6.0), b], [], 16, 4, {0: True, 1: True, 2: True, 3: True})
    case("one_object_point", [], [a], 16, 4, {0: True})
    case("one_scan_point", [a], [], 16, 4, {0: True})
    # above / below the field of view: clamped into rows 0 and H - 1, where they meet in-view points of the same column
    up, down = P(4, 0, 3.0, pitch=FOV[0] + 0.3), P(11, 0, 3.0, pitch=FOV[1] - 0.3)
    case("clamped_rows", [P(4, 0, 5.0), P(11, 3, 5.0), P(4, 1, 5.0)], [up, down], 16, 4, {0: False, 1: False, 2: True, 3: True, 4: True},
         clamped={3: 0, 4: 3})
    # the axes with fov = 1 (exact pixel arithmetic): +x -> column W/2, +y -> W/4, -y -> 3W/4, (-1, +0.0) -> 0, (-1, -0.0) -> W-1
    axes = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (-1.0, 0.0, 0.0), (-1.0, -0.0, 0.0)]
    for W, H in ((16, 4), (64, 8)):
        case(f"axes_{W}x{H}", axes, [tuple(2 * v for v in p) for p in axes], W, H,
             {**{i: True for i in range(5)}, **{5 + i: False for i in range(5)}}, fov=FOV_EXACT,
             exact_cols=[W // 2, W // 4, 3 * W // 4, 0, W - 1] * 2, exact_row=H // 4)
    # 257 points at the centres of random pixels of the 64x8 image, 100 of them repeated (bit-equal depths), 120 object points
    rng = _rng(9)
    base = [range_point(int(rng.integers(0, 64)), int(rng.integers(0, 8)), float(rng.integers(8, 24)) / 4, 64, 8, *FOV) for _ in range(157)]
    pts = base + [base[i] for i in rng.integers(0, 157, 100)]
    pts = [pts[i] for i in rng.permutation(257)]
    case("random_257", pts[:137], pts[137:], 64, 8)
    return out


# ------------------------------------------------------------------------------------------------ mopa_voxelize_f64
def ref_voxelize_f64(pts, keep_in, R, scale, full_scale, u, batch):
    """augment_and_scale_3d on the rows with keep_in != 0 plus post_process's field filter, for all rows at once:
    -> (coords (n, 4) int64 [x, y, z, batch], keep (n,) bool).  R None = no rotation, u None = no translation.  The coordinates
    of rows with keep_in == 0 mean nothing; with no row kept at all they are zero."""
    n = len(pts)
    kin = np.ones(n, bool) if keep_in is None else np.asarray(keep_in) != 0
    coords = np.zeros((n, 4), np.int64)
    coords[:, 3] = batch
    if not kin.any():
        return coords, np.zeros(n, bool)
    c = np.round((pts if R is None else pts @ R) * scale)
    c = c - c[kin].min(0)
    if u is not None:
        c = c + np.clip(full_scale - c[kin].max(0) - 0.001, 0, None) * u
    keep = kin & (c.min(1) >= 0) & (c.max(1) < full_scale)
    coords[:, :3] = c.astype(np.int64)
    return coords, keep


def reference_rot_matrix(noisy_rot=0.0, flip_x=0.0, flip_y=0.0, rot_z=0.0):
    """The rotation of the 3D augmentation, drawn from numpy's global RNG: noise on the identity (float32), the flips' signs, the
    angle about z."""
    if not (noisy_rot > 0 or flip_x > 0 or flip_y > 0 or rot_z > 0):
        return None
    r = np.eye(3, dtype=np.float32)
    if noisy_rot > 0:
        r += np.random.randn(3, 3) * noisy_rot
    if flip_x > 0:
        r[0][0] *= np.random.randint(0, 2) * 2 - 1
    if flip_y > 0:
        r[1][1] *= np.random.randint(0, 2) * 2 - 1
    if rot_z > 0:
        t = np.random.rand() * rot_z
        r = r.dot(np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]], dtype=np.float32))
    return r


def voxel_cases():
    """name -> dict(pts (n, 3) float64, keep_in (n,) uint8 or None, R (3, 3) float64 or None, scale, full_scale, u (3,) or None, batch)."""
    out = {}
    rng = _rng(21)

    def case(name, pts, scale, full_scale, keep_in=None, R=None, u=None, batch=0):
        out[name] = dict(pts=np.ascontiguousarray(pts, np.float64), keep_in=None if keep_in is None else np.asarray(keep_in, np.uint8),
                         R=None if R is None else np.ascontiguousarray(R, np.float64), scale=scale, full_scale=full_scale,
                         u=None if u is None else np.asarray(u, np.float64), batch=batch)

    cloud = rng.integers(int(-3 * Q), int(3 * Q), (700, 3)) / Q
    case("no_rotation", cloud, 20, 4096, batch=5)
    case("one_point", cloud[:1], 20, 4096, batch=1)
    case("flip_x", cloud, 20, 4096, R=np.diag([-1.0, 1.0, 1.0]))
    case("flip_y", cloud, 20, 4096, R=np.diag([1.0, -1.0, 1.0]), batch=2)
    case("flip_xy", cloud, 20, 4096, R=np.diag([-1.0, -1.0, 1.0]))
    k = np.arange(-40, 41)
    ties = np.stack([(k + 0.5) / 16, (k[::-1] + 0.5) / 16, (rng.permutation(k) + 0.5) / 16], 1)      # scaled: k + 0.5, k < 0 and k > 0
    case("ties_scale_16", ties, 16, 4096)
    case("ties_scale_16_flip", ties, 16, 4096, R=np.diag([-1.0, 1.0, 1.0]), keep_in=(np.arange(81) % 3 != 0))
    case("keep_partly_zero", cloud, 20, 4096, keep_in=rng.integers(0, 2, 700), batch=3)
    # the extreme points are culled: minimum and maximum are those of the kept rows only
    far = np.concatenate([cloud, [[-50.0, 60.0, -70.0], [80.0, -90.0, 100.0]]], 0)
    case("keep_culls_the_extremes", far, 20, 4096, keep_in=np.r_[np.ones(700, np.uint8), 0, 0], u=[0.25, 0.5, 0.75])
    case("keep_all_zero", cloud, 20, 4096, keep_in=np.zeros(700, np.uint8), u=[0.25, 0.5, 0.75])
    small = rng.integers(int(-1 * Q), int(1 * Q) + 1, (500, 3)) / Q
    small[0], small[1] = -1.0, 1.0                          # extent 2 m * 16 = 32 < 64
    case("translation_extent_below_field", small, 16, 64, u=[0.25, 0.5, 0.9375], batch=4)
    case("translation_u_zero_and_almost_one", small, 16, 64, u=[0.0, 1.0 - 2.0 ** -53, 0.5])
    wide = rng.integers(int(-3 * Q), int(3 * Q) + 1, (500, 3)) / Q
    wide[0], wide[1] = -3.0, 3.0                            # extent 6 m * 16 = 96 > 64: the offset clips to 0
    case("translation_extent_above_field", wide, 16, 64, u=[0.25, 0.5, 0.9375])
    # without translation: coordinates 0 (the minimum itself), full_scale - 1 and exactly full_scale
    edge = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [3.9375, 3.9375, 3.9375], [0.0, 4.0, 0.0], [0.0, 0.0, 4.0], [1.0, 2.0, 3.0]])
    case("coordinate_exactly_full_scale", edge, 16, 64, batch=7)
    # one seeded noisy rotation on unquantised points: the comparison holds as long as no scaled coordinate is within 1e-9 of a tie
    st = np.random.get_state()
    np.random.seed(4242)
    R = reference_rot_matrix(0.1, 0.0, 0.5, 6.2831)
    u = np.random.rand(3)
    np.random.set_state(st)
    case("noisy_rotation", rng.normal(0.0, 12.0, (1000, 3)), 20, 4096, R=R.astype(np.float64), u=u, keep_in=rng.random(1000) < 0.9)
    return out


def g8_post_process(k, g8):
    """locs (m, 4) int64 of fixture G8's post_process run of case k, recomputed with ref_voxelize_f64: the reference's cloud
    (scan + G8's placed object), its occlusion culling (oracle), its draws (seed 200 + k), then the restatement."""
    from oracle.gen_golden import vgi_case
    c = vgi_case(k)
    n0 = len(c["ori_pc"])
    cat = np.concatenate([c["ori_pc"][:, :3].astype(np.float64), g8[f"obj_xyz{k}"]], 0)
    mask = np.zeros(len(cat), bool)
    mask[n0:] = True
    valid = ovgi.range_keep(cat, mask, 0.05235, -0.43633, 1024, 64)
    st = np.random.get_state()
    np.random.seed(200 + k)
    R = reference_rot_matrix(0.1, 0.0, 0.5, 6.2831)
    u = np.random.rand(3)
    np.random.set_state(st)
    coords, keep = ref_voxelize_f64(cat, valid, R.astype(np.float64), 20, 4096, u, 0)
    return coords[keep], valid


# ------------------------------------------------------------------------------------------------ Python level
OVERLAP_VOXEL_SIZES = [0.5, 0.25, 0.2, 0.3]
OVERLAP_RANGE = (2.5, 2.5)
PAIR = np.array([[1.3, 1.05, -1.95], [1.4, 1.05, -1.95]], np.float32)      # one float64 voxel at 0.2, two float32 floors (6 and 7)


def split_value(vs, lo=3, hi=40):
    """(a, b) float32 in one float64 voxel where b's float32 floor is another cell than its float64 floor and a's is not, or
    None (a power-of-two voxel size)."""
    for k in range(lo, hi):
        b0 = np.float32(k * vs)
        for b in (b0, np.nextafter(b0, np.float32(-np.inf)), np.nextafter(b0, np.float32(np.inf))):
            v64 = np.floor(np.float64(b) / vs)
            if np.floor(b / np.float32(vs)) != v64:
                return np.float32((v64 + 0.5) * vs), b
    return None


def overlap_cloud(vs, seed=0, n=1500):
    """-> (scan (n, 3) float32, obj (m, 3) float32): the two-point case in both orders (second time mirrored in y), 700 points
    whose coordinates are float32(k * vs) or one of its float32 neighbours, random points; the object is a small cluster inside
    one voxel plus, where the voxel size allows it, split_value's two points in front.  (Not quantised to 2^-10: this case is about float32 against float64 quotients.)"""
    rng = _rng(seed + int(vs * 1000))
    swapped = PAIR[::-1] * np.array([1, -1, 1], np.float32)

    def near_faces(m, lo, hi):
        k = rng.integers(lo, hi, (m, 3))
        v = (k * vs).astype(np.float32)
        step = rng.integers(-1, 2, (m, 3))
        v = np.where(step < 0, np.nextafter(v, np.float32(-np.inf)), np.where(step > 0, np.nextafter(v, np.float32(np.inf)), v))
        return v.astype(np.float32)

    sr = int(OVERLAP_RANGE[0] / vs)
    faces = near_faces(700, -sr - 1, 2 * sr + 2)
    faces[:, 2] = near_faces(700, -12, 6)[:, 2]
    rest = np.stack([rng.uniform(-3.0, 9.0, n - 704), rng.uniform(-6.0, 6.0, n - 704), rng.uniform(-4.0, 6.0, n - 704)], 1).astype(np.float32)
    scan = np.concatenate([PAIR, swapped, faces, rest], 0)
    y0, z0 = 10.5 * vs, 0.5 * vs
    ab = split_value(vs)
    x0 = 2.5 * vs if ab is None else float(ab[0])
    obj = np.stack([rng.uniform(x0 - 0.3 * vs, x0 + 0.3 * vs, 12), rng.uniform(y0 - 0.2 * vs, y0 + 0.2 * vs, 12),
                    rng.uniform(z0 - 0.2 * vs, z0 + 0.2 * vs, 12)], 1).astype(np.float32)
    if ab is not None:      # b comes behind a point of its own float64 voxel: the reference never looks at b's float32 floor
        obj = np.concatenate([[[ab[0], y0, z0], [ab[1], y0, z0]], obj], 0).astype(np.float32)
    return scan, obj


def free_cells_objects():
    """name -> (obj (m, 3) float64, z_max or None) on the map of MAPS['vs0.5_x'] (16 x 16 cells): does the box fit the grid?"""
    def span(ex, ey, ez):
        return np.array([[1.0, 1.0, -1.0], [1.0 + ex * 0.5, 1.0 + ey * 0.5, -1.0 + ez * 0.5]])
    return {"fits": (span(2, 2, 2), None),
            "box_equals_the_map": (span(10, 10, 1), None),              # ceil(sqrt(11^2 + 11^2)) = 16 cells
            "wider_than_the_map": (span(11, 11, 1), None),              # ceil(sqrt(12^2 + 12^2)) = 17 cells
            "taller_than_the_slab": (span(2, 2, 5), -7.0),              # Z = 7 + (-7) - (-4) = 4 slots under a box of 6
            "as_tall_as_the_slab": (span(2, 2, 5), -5.0)}               # Z = 6 slots, the box's height: one layer of cells
