"""The inputs and numpy references of tests/test_gpu_vgi_edges.py are what that file takes them for (no GPU needed): every
restatement agrees with oracle/vgi.py where that has the function, the float64 voxeliser's restatement reproduces fixture G8,
and every case holds the edge it is named after -- the condition under which the device tests mean anything."""
import os

import numpy as np
import pytest

import _vgi_cases as vc
from oracle import vgi as ovgi

INT_MAX = vc.INT_MAX


def _on_grid(a):
    """Every value is a multiple of 2^-10."""
    return bool((np.asarray(a, np.float64) * vc.Q == np.round(np.asarray(a, np.float64) * vc.Q)).all())


# ------------------------------------------------------------------------------------------------ first points
@pytest.mark.parametrize("name", list(vc.MAPS))
def test_first_cloud_holds_its_edges(name):
    vs, sr, front = vc.MAPS[name]
    g = vc.map_geometry(vs, sr, front)
    pts, names = vc.first_cloud(vs, sr, front)
    assert pts.dtype == np.float32 and len(pts) == 3000 and _on_grid(pts)
    assert names.pop("dup_last") == 2999 and max(names.values()) < 62             # a prefix of 63 rows holds every edge
    names["dup_last"] = 62
    assert np.array_equal(vc.first_cloud(vs, sr, front, 63)[0][62], pts[names["dup_a"]])
    names["dup_last"] = 2999
    c = vc.voxel_f32(pts, vs) - np.array([g["ox"], g["oy"], g["zlo"]])
    f, l = (0, 1) if front == "x" else (1, 0)
    F, L = (g["X"], g["Y"]) if front == "x" else (g["Y"], g["X"])
    r = names
    assert pts[r["neg_face"], l] == -vs and pts[r["neg_face"], 2] == -vs and c[r["neg_face"], l] == L // 2 - 1 and c[r["neg_face"], 2] == -1 - vc.ZLO
    assert np.array_equal(pts[r["dup_a"]], pts[r["dup_b"]]) and np.array_equal(pts[r["dup_a"]], pts[r["dup_last"]])
    assert (c[r["f_first"], f], c[r["f_below"], f], c[r["f_last"], f], c[r["f_out"], f]) == (0, -1, F - 1, F)
    assert (c[r["l_first"], l], c[r["l_below"], l], c[r["l_last"], l], c[r["l_out"], l]) == (0, -1, L - 1, L)
    assert (c[r["z_slot0"], 2], c[r["z_below"], 2], c[r["z_slot127"], 2], c[r["z_slot128"], 2]) == (0, -1, 127, 128)
    for k in ("f_first", "f_out"):                       # exactly on a face: the quotient is an integer
        assert pts[r[k], f] / np.float32(vs) == np.floor(pts[r[k], f] / np.float32(vs))
    for k in ("z_below", "z_slot128"):                   # dropped by z, inside in x and y
        assert 0 <= c[r[k], 0] < g["X"] and 0 <= c[r[k], 1] < g["Y"]
    assert c[r["xy_out_z_out"], f] < 0 and c[r["xy_out_z_out"], 2] < 0
    first, status = vc.ref_first_points(pts, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"])
    vol = first.reshape(g["X"], g["Y"], vc.ZR)
    assert vol[tuple(c[r["dup_a"]])] == r["dup_a"] and status == 0       # the smaller index wins
    assert (vol != INT_MAX).sum() > 400 and (np.bincount(vol[vol != INT_MAX], minlength=3000) == 0).sum() > 300   # many voxels, many later points
    masks, dropped = vc.first_masks(pts, vs, g)
    assert dropped[r["z_below"]] and dropped[r["z_slot128"]] and not dropped[r["xy_out_z_out"]]
    assert (masks["ground_dropped"][dropped] != 0).sum() == 1 and not masks["nonground_dropped"][dropped].any()
    assert masks["nonground_dropped"][r["xy_out_z_out"]] == 1 and masks["nonground_dropped"].sum() > 100
    assert vc.ref_first_points(pts, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], masks["ground_dropped"])[1] == 1
    assert vc.ref_first_points(pts, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], masks["nonground_dropped"])[1] == 0


@pytest.mark.parametrize("name", list(vc.MAPS))
@pytest.mark.parametrize("n", vc.FIRST_SIZES)
def test_first_points_reference_is_the_oracles_grid_and_representatives(name, n):
    """Occupancy == overlap_grid's grid over its slab; the stored index == sparse_quantize's representative of that voxel."""
    vs, sr, front = vc.MAPS[name]
    g = vc.map_geometry(vs, sr, front)
    pts, _ = vc.first_cloud(vs, sr, front, n)
    first, _ = vc.ref_first_points(pts, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"])
    vol = first.reshape(g["X"], g["Y"], vc.ZR)
    obj = np.array([[1.0, 1.0, 0.0], [1.0 + 2 * vs, 1.0 + vs, 3 * vs]])
    o = ovgi.overlap_grid(pts, obj, vs, sr, -2.0, None, front)
    z0 = int(np.floor(-2.0 / vs)) - g["zlo"]
    assert o["grid"].shape[:2] == (g["X"], g["Y"]) and tuple(o["offset"][:2]) == (g["ox"], g["oy"])
    assert np.array_equal(vol[:, :, z0:z0 + o["grid"].shape[2]] != INT_MAX, o["grid"] != 0)
    vox, idx = ovgi.sparse_quantize(pts[:, :3], vs, return_index=True)
    c = vox.astype(np.int64) - np.array([g["ox"], g["oy"], g["zlo"]])
    inside = (c >= 0).all(1) & (c[:, 0] < g["X"]) & (c[:, 1] < g["Y"]) & (c[:, 2] < vc.ZR)
    assert inside.sum() == (vol != INT_MAX).sum()
    assert np.array_equal(vol[c[inside, 0], c[inside, 1], c[inside, 2]], idx[inside])


@pytest.mark.parametrize("vs", vc.OVERLAP_VOXEL_SIZES)
def test_overlap_cloud_tells_the_two_quotients_apart(vs):
    """The representatives' reference IS the oracle's grid at every voxel size; at 0.2 and 0.3 marking every point at its float32
    floor is not (grid and box both differ), at the powers of two it is."""
    scan, obj = vc.overlap_cloud(vs)
    g = vc.map_geometry(vs, vc.OVERLAP_RANGE, "x")
    assert len(scan) == 1500 and np.array_equal(scan[:2], vc.PAIR) and np.array_equal(scan[2:4, 0], vc.PAIR[::-1, 0])
    o = ovgi.overlap_grid(scan, obj, vs, vc.OVERLAP_RANGE, -2.0, None, "x")
    z0 = int(np.floor(-2.0 / vs)) - g["zlo"]
    Z = o["grid"].shape[2]
    rep = vc.ref_first_points_rep(scan, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"]).reshape(g["X"], g["Y"], vc.ZR)
    every = vc.ref_first_points(scan, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"])[0].reshape(g["X"], g["Y"], vc.ZR)
    assert np.array_equal(rep[:, :, z0:z0 + Z] != INT_MAX, o["grid"] != 0)
    ov = np.floor(obj / vs)
    ext = ov.max(0) - ov.min(0) + 1
    box_every = np.ceil(np.sqrt(ext[0] ** 2 + ext[1] ** 2))
    differs = not np.array_equal(every[:, :, z0:z0 + Z] != INT_MAX, o["grid"] != 0)
    near = scan[4:704]
    assert (np.abs(near.astype(np.float64) - np.round(near.astype(np.float64) / vs) * vs) < 1e-6).all()      # within an ulp or so of k * vs
    if vs in (0.2, 0.3):
        assert differs and box_every != o["box"][0] and vc.split_value(vs) is not None
        assert ((vc.voxel_f32(scan, vs) != vc.voxel_f64(scan, vs)).any(1)).sum() > 100
    else:
        assert not differs and box_every == o["box"][0] and vc.split_value(vs) is None
    assert 0 < o["free"].sum() < o["free"].size                    # the comparison of the centres is not one of two Nones
    if vs == 0.2:                                                    # the two-point case alone, both orders, at check_overlap's default arguments
        a = ovgi.overlap_grid(vc.PAIR, np.array([[5, 5, 0], [5.1, 5.1, 0.1]]), 0.2, (25.0, 25.0), -2.0, None, "x")["grid"]
        b = ovgi.overlap_grid(vc.PAIR[::-1], np.array([[5, 5, 0], [5.1, 5.1, 0.1]]), 0.2, (25.0, 25.0), -2.0, None, "x")["grid"]
        assert np.argwhere(a).tolist() == [[6, 130, 0]] and np.argwhere(b).tolist() == [[7, 130, 0]]


# ------------------------------------------------------------------------------------------------ box free
def test_box_reference_is_the_oracles_window_sum():
    """On clouds and objects (square boxes, the circumscribed circle) ref_box_free over ref_first_points == overlap_grid's free."""
    for name in ("vs0.5_x", "vs0.25_y", "vs1_x", "vs0.5_x_rect"):
        seen = set()
        vs, sr, front = vc.MAPS[name]
        g = vc.map_geometry(vs, sr, front)
        pts, _ = vc.first_cloud(vs, sr, front, 400, seed=3)
        first, _ = vc.ref_first_points(pts, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"])
        for ex, ey, ez in ((0, 0, 0), (1, 0, 1), (2, 2, 3), (5, 4, 0)):
            obj = np.array([[1.0, 1.0, 0.0], [1.0 + ex * vs, 1.0 + ey * vs, ez * vs]])
            o = ovgi.overlap_grid(pts, obj, vs, sr, -2.0, None, front)
            if min(o["free"].shape) == 0:
                continue
            free = vc.ref_box_free(first, g["X"], g["Y"], g["zlo"], int(np.floor(-2.0 / vs)), o["grid"].shape[2], *[int(b) for b in o["box"]])
            assert np.array_equal(free != 0, o["free"]), (name, ex, ey, ez)
            seen |= set(np.unique(free).tolist())
        assert seen == {0, 1}, name


def test_box_cases_hold_their_edges():
    cs = vc.box_cases()
    X, Y = vc.BOX_X, vc.BOX_Y
    free = {k: vc.ref_box_free(c["first"], c["X"], c["Y"], c["zlo"], c["gz0"], c["Z"], *c["box"]) for k, c in cs.items()}
    for k, c in cs.items():
        bx, by, bz = c["box"]
        assert free[k].shape == (X - bx + 1, Y - by + 1, c["Z"] - bz + 1), k
        assert (c["first"] != INT_MAX).any() and c["first"].min() == 0            # point index 0 is an occupied voxel, not an empty one
    assert free["bx_eq_X"].shape[0] == 1 and free["bx_by_eq_XY"].shape[:2] == (1, 1) and free["bz_eq_Z"].shape[2] == 1
    for k in ("bx_eq_X", "bx_by_eq_XY", "bz_eq_Z", "box_1x1x1", "sparse", "slab_at_slot_0", "slab_to_slot_128", "whole_volume", "full_column"):
        assert 0 < free[k].sum() < free[k].size, k                                   # both answers occur
    assert free["box_eq_grid_free"].tolist() == [[[1]]] and free["box_eq_grid_taken"].tolist() == [[[0]]]
    assert free["empty_grid"].all()
    assert np.array_equal(free["box_1x1x1"] == 0, (cs["box_1x1x1"]["first"].reshape(X, Y, vc.ZR) != INT_MAX)[:, :, 60:68])
    col = free["full_column"]
    assert not col[4:6, 2:5].any() and col.sum() == col.size - 2 * 3 * col.shape[2]
    e = free["eight_corners"]                       # every corner cell of the output is taken, everything else is free
    corners = [(x, y, z) for x in (0, e.shape[0] - 1) for y in (0, e.shape[1] - 1) for z in (0, e.shape[2] - 1)]
    assert all(e[c] == 0 for c in corners) and e.sum() == e.size - 8
    assert cs["slab_at_slot_0"]["gz0"] == vc.ZLO and cs["slab_to_slot_128"]["gz0"] + cs["slab_to_slot_128"]["Z"] == vc.ZLO + vc.ZR
    for k, (X_, Y_, gz0, Z, bx, by, bz) in vc.BOX_REFUSED.items():
        assert min(X_, Y_, Z, bx, by, bz) <= 0 or bx > X_ or by > Y_ or bz > Z or gz0 < vc.ZLO or gz0 + Z > vc.ZLO + vc.ZR, k


def test_free_cells_objects_fit_or_not_as_named():
    vs, sr, front = vc.MAPS["vs0.5_x"]
    pts, _ = vc.first_cloud(vs, sr, front, 300)
    shapes = {k: ovgi.overlap_grid(pts, obj, vs, sr, -2.0, z_max, front) for k, (obj, z_max) in vc.free_cells_objects().items()}
    assert min(shapes["fits"]["free"].shape) > 1
    assert shapes["box_equals_the_map"]["box"][0] == 16 and shapes["box_equals_the_map"]["free"].shape[:2] == (1, 1)
    assert shapes["wider_than_the_map"]["box"][0] == 17 and shapes["wider_than_the_map"]["free"].size == 0
    t = shapes["taller_than_the_slab"]
    assert t["box"][2] > t["grid"].shape[2] > 0 and t["box"][0] <= 16 and t["free"].size == 0
    t = shapes["as_tall_as_the_slab"]
    assert t["box"][2] == t["grid"].shape[2] and t["free"].shape[2] == 1


# ------------------------------------------------------------------------------------------------ ground columns, road height
def _cells_of(g):
    cx, cy = np.meshgrid(np.arange(g["X"]) + g["ox"], np.arange(g["Y"]) + g["oy"], indexing="ij")
    return np.stack([cx.reshape(-1), cy.reshape(-1)], 1)


def test_ground_cloud_holds_its_edges_and_agrees_with_the_oracle():
    pts, flags, g = vc.ground_cloud()
    vs = g["vs"]
    assert _on_grid(pts) and len(pts) == 3000
    first, status = vc.ref_first_points(pts, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], flags)
    g2d = vc.ref_ground_cells(first, flags, g["X"], g["Y"]).reshape(g["X"], g["Y"])
    vol = first.reshape(g["X"], g["Y"], vc.ZR)
    C = vc.GROUND_CELLS
    col = {k: vol[c[0] - g["ox"], c[1] - g["oy"]] for k, c in C.items()}
    is_g = {k: [(z, bool(flags[i])) for z, i in enumerate(col[k]) if i != INT_MAX] for k in C}
    assert status == 0
    assert [z for z, f in is_g["top"] if f] == [127] and len(is_g["top"]) == 3
    assert {f for _, f in is_g["mixed"]} == {True, False}
    assert is_g["late"] == [(-1 - vc.ZLO, False)] and is_g["early"] == [(-1 - vc.ZLO, True)]
    v = vc.voxel_f32(pts, vs)
    for k, want in (("late", [0, 1]), ("early", [1, 0])):          # one voxel, two points, the flags in this order
        rows = np.nonzero((v[:, :2] == C[k]).all(1))[0]
        assert flags[rows].tolist() == want and len(set(v[rows, 2])) == 1
    assert [z for z, f in is_g["two"] if f] == [-3 - vc.ZLO, 1 - vc.ZLO]
    low = (v == (*C["two"], -3)).all(1)
    assert low.sum() > 900 and 0 < flags[low].sum() < low.sum() and flags[0] == 1 and low[0]       # shared with non-ground points
    assert low[:1023].sum() < low[:1025].sum() or low[:1025].sum() < low.sum()
    assert [int(g2d[c[0] - g["ox"], c[1] - g["oy"]]) for c in (C["top"], C["mixed"], C["late"], C["early"], C["two"])] == [1, 1, 0, 1, 1]
    assert 0 < g2d.sum() < g2d.size
    # the oracle: ground cells = the (x, y) of the voxels whose representative is ground
    cells = _cells_of(g)
    centres = np.concatenate([(cells + 0.5) * vs, np.zeros((len(cells), 1))], 1)
    for n in vc.ROAD_SIZES:
        p, f = pts[:n], flags[:n]
        fi, _ = vc.ref_first_points(p, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], f)
        want, voxel_pc, gm, pc_inv = ovgi.ground_centers(p, centres, f, vs)
        ref = vc.ref_ground_cells(fi, f, g["X"], g["Y"])
        assert np.array_equal(cells[ref != 0], want.astype(np.int64)), n
        # road height: the oracle's choice of the voxel (placement: the lowest ground voxel of the cell) and of its points
        for cell in cells[ref != 0][:: max(1, int(ref.sum()) // 12)].tolist() + [list(C["two"])]:
            cur = gm.copy()
            cur[cur] = (voxel_pc[gm][:, 0] == cell[0]) & (voxel_pc[gm][:, 1] == cell[1])
            inter = np.where(cur)[0]
            if inter.shape[0] > 1:
                inter = inter[np.argmin(voxel_pc[inter, 2], axis=0)]
            z = p[np.where(pc_inv == inter)[0], 2].astype(np.float64)
            assert vc.ref_road_height(p, vs, fi, f, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], cell) == (float(z.sum()), float(len(z))), (n, cell)
    assert vc.ref_road_height(pts, vs, first, flags, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], C["late"]) == (0.0, 0.0)
    s, c = vc.ref_road_height(pts, vs, first, flags, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], C["two"])
    assert c == low.sum() and s * vc.Q == round(s * vc.Q)


# ------------------------------------------------------------------------------------------------ candidates
@pytest.mark.parametrize("name", list(vc.cand_cases()))
def test_candidate_cases_agree_with_the_oracle_and_hold_their_edges(name):
    c = vc.cand_cases()[name]
    g = c["g"]
    first, status = vc.ref_first_points(c["scan"], c["vs"], g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], c["g_mask"])
    g2d = vc.ref_ground_cells(first, c["g_mask"], g["X"], g["Y"])
    ref = vc.ref_candidates(c["free"], c["ext"], c["off"], c["vs"], c["ori_range"], c["P"], c["image_size"], g2d, g["ox"], g["oy"], g["X"], g["Y"])
    ora = vc.oracle_candidates(c)
    assert status == 0 and np.array_equal(ref[0], ora[0]) and ref[1] == ora[1]
    cen = vc.cand_centres(c)
    assert _on_grid(cen * 256) and (cen * 4 == np.round(cen * 4)).all()                       # multiples of 0.25
    u, v, p2 = vc.cand_projection(c, cen) if len(cen) else (np.zeros(0),) * 3
    kept = {tuple(r) for r in ovgi.filter_centers(cen, c["obj"], c["P"], c["image_size"]).tolist()} if len(cen) else set()
    front_ok = cen[:, 0] > 0 if len(cen) else np.zeros(0, bool)
    w, h = c["image_size"]

    def some(mask):
        assert mask.any(), name
        return [tuple(r) for r in cen[mask].tolist()]

    if name.startswith("image_bounds"):
        assert c["ori_range"] == 0.0
        assert not any(r in kept for r in some(cen[:, 0] == 0))                                # cx == 0 is out
        edges = [u == w, v == 0, v == h] + ([u == 0] if name.endswith("_x") else [])
        for e in edges:                                                                         # exactly on the image's border: out
            assert not any(r in kept for r in some(front_ok & e))
        inside = front_ok & (u > 0) & (u < w) & (v > 0) & (v < h)
        assert all(r in kept for r in some(inside)) and len(kept) == inside.sum()
        # one cell further inside than a border centre is in
        step = c["vs"]
        borders = [(u == w, 1 if name.endswith("_x") else 0, 1 if name.endswith("_x") else -1), (v == 0, 2, -1), (v == h, 2, 1)]
        if name.endswith("_x"):             # front y: u == 0 needs cx == -cy < 0, which the first filter has already removed
            borders.append((u == 0, 1, -1))
        for e, axis, sign in borders:
            moved = [tuple(np.add(r, np.eye(3)[axis] * sign * step)) for r in some(front_ok & e)]
            assert any(m in kept for m in moved), (name, axis)
    if name.startswith("range_345"):
        rng_ = np.sqrt(cen[:, 0] ** 2 + cen[:, 1] ** 2)
        assert c["ori_range"] == 2.5
        on = some(front_ok & (rng_ == 2.5) & (u > 0) & (u < w) & (v > 0) & (v < h))
        assert all(r in kept for r in on) and {(abs(r[0]), abs(r[1])) for r in on} & {(2.0, 1.5), (1.5, 2.0)}
        assert not any(r in kept for r in some(front_ok & (rng_ < 2.5) & (u > 0) & (u < w) & (v > 0) & (v < h)))
    if name == "behind_camera_x":
        assert (p2 != 0).all() and kept == set(some(front_ok & (p2 < 0))) and (front_ok & (p2 > 0)).any()
    if name == "every_cell_passes":
        assert ref[1] == (c["free"].size, c["free"].size) and ref[0].reshape(16, 16)[:15, :15].all() and ref[0].sum() == 225
    if name == "no_free_cell":
        assert ref[1] == (0, 0) and not ref[0].any()
    if name == "cells_not_ground":
        assert ref[1] == (c["free"].size, c["free"].size) and ref[0].sum() == 225 - 4 and g2d.sum() == 256 - 4
    if name.startswith("random_free"):
        assert 0 < ref[1][1] < ref[1][0] < c["free"].size and 0 < ref[0].sum()
        full = vc.ref_candidates(c["free"], c["ext"], c["off"], c["vs"], c["ori_range"], c["P"], c["image_size"], np.ones_like(g2d), g["ox"], g["oy"],
                                 g["X"], g["Y"])
        assert full[0].sum() > ref[0].sum()                                                     # a passing centre over a hole


# ------------------------------------------------------------------------------------------------ compaction
def test_compact_reference_is_np_unique_order():
    for X, Y in vc.COMPACT_MAPS:
        for fill in vc.COMPACT_FILLS:
            cand = vc.compact_input(X, Y, fill)
            cells, n = vc.ref_compact(cand, X, Y, -5, 7)
            want = {"none": 0, "all": X * Y, "last": 1, "every65": (X * Y + 64) // 65}[fill]
            assert n == want == len(cells)
            if n:
                assert np.array_equal(cells, np.unique(cells[::-1], axis=0)) and cells[-1].tolist() != [] and cells.dtype == np.int32
            if fill == "last":
                assert cells.tolist() == [[X - 1 - 5, Y - 1 + 7]]
    assert sorted(X * Y for X, Y in vc.COMPACT_MAPS) == [1, 1023, 1024, 1025, 2049]


# ------------------------------------------------------------------------------------------------ range image
@pytest.mark.parametrize("name", list(vc.range_cases()))
def test_range_cases_agree_with_the_oracle_and_hold_their_edges(name):
    c = vc.range_cases()[name]
    pts, n0, W, H = c["pts"], c["n_scan"], c["W"], c["H"]
    assert _on_grid(pts) and np.isfinite(pts).all()
    mask = np.arange(len(pts)) >= n0
    ref = vc.ref_range_keep(pts, n0, c["fov_up"], c["fov_down"], W, H)
    if mask.any():
        assert np.array_equal(ref, ovgi.range_keep(pts, mask, c["fov_up"], c["fov_down"], W, H))
    else:                                  # post_process does not project a cloud without object points: everything stays
        assert ref.all()
    for row, kept in c["expect"].items():
        assert bool(ref[row]) == kept, (name, row)
    py, px, depth = ovgi.range_pixels(pts, c["fov_up"], c["fov_down"], W, H)
    assert (depth > 0).all()
    rx, ry, _ = vc.range_real_pixels(pts, c["fov_up"], c["fov_down"], W, H)
    if "exact_cols" in c:
        # the axes: the pixel arithmetic is exact, the points lie ON pixel faces (column k.0, row H/4 .0), -0.0 apart from +0.0
        assert px.tolist() == c["exact_cols"] and (py == c["exact_row"]).all() and (ry == c["exact_row"]).all()
        assert rx[:5].tolist() == [W / 2, W / 4, 3 * W / 4, 0.0, float(W)]
        assert np.signbit(pts[4, 1]) and not np.signbit(pts[3, 1]) and np.signbit(pts[9, 1])
    else:
        # everything else sits near the centre of its pixel (or far outside the rows): no libm's last bit moves it
        fx, fy = rx - np.floor(rx), ry - np.floor(ry)
        assert ((fx > 0.4) & (fx < 0.6)).all()
        inside = (ry > 0) & (ry < H)
        assert ((fy[inside] > 0.4) & (fy[inside] < 0.6)).all() and ((ry[~inside] < -1) | (ry[~inside] > H + 1)).all()
    for i, j in c.get("ties", []):
        assert depth[i].tobytes() == depth[j].tobytes() and (py[i], px[i]) == (py[j], px[j])
    for row, want in c.get("clamped", {}).items():
        assert py[row] == want and not 0 <= ry[row] < H
    if name == "random_257":
        assert len(pts) == 257
        pix = py * W + px
        objpix = np.isin(pix, pix[n0:])
        tied = sum(1 for q in np.unique(pix[objpix]) if (depth[pix == q] == depth[pix == q].min()).sum() > 1)
        assert tied > 10 and 0 < ref.sum() < 257 and (~objpix).sum() > 10


# ------------------------------------------------------------------------------------------------ float64 voxeliser
@pytest.mark.parametrize("name", list(vc.voxel_cases()))
def test_voxel_cases_hold_their_edges(name):
    c = vc.voxel_cases()[name]
    coords, keep = vc.ref_voxelize_f64(c["pts"], c["keep_in"], c["R"], c["scale"], c["full_scale"], c["u"], c["batch"])
    assert coords.shape == (len(c["pts"]), 4) and (coords[:, 3] == c["batch"]).all()
    q = (c["pts"] if c["R"] is None else c["pts"] @ c["R"]) * c["scale"]
    frac = np.abs(q - np.floor(q) - 0.5)
    kin = np.ones(len(keep), bool) if c["keep_in"] is None else c["keep_in"] != 0
    assert not keep[~kin].any()
    if name != "noisy_rotation":
        assert _on_grid(c["pts"])
    if name.startswith("ties_scale_16"):
        assert (frac == 0).all() and (q > 0).any() and (q < 0).any()                       # every scaled coordinate is k + 0.5
        assert (np.round(q) % 2 == 0).all()                                                 # ties go to even
    if name == "keep_all_zero":
        assert not keep.any()
    if name == "keep_partly_zero":
        assert 0 < kin.sum() < len(kin) and np.array_equal(keep, kin)
    if name == "keep_culls_the_extremes":
        full = vc.ref_voxelize_f64(c["pts"], None, c["R"], c["scale"], c["full_scale"], c["u"], c["batch"])[0]
        assert not np.array_equal(full[:700], coords[:700]) and keep[:700].all()
    if name == "translation_extent_below_field":
        ext = np.round(c["pts"] * 16).max(0) - np.round(c["pts"] * 16).min(0)
        assert (ext == 32).all() and keep.all() and (coords[:, :3].min(0) > 0).all()         # moved off the origin, still inside
    if name == "translation_u_zero_and_almost_one":
        assert coords[:, 0].min() == 0 and coords[:, 1].max() == 63 and keep.all()
    if name == "translation_extent_above_field":
        assert (coords[:, :3].min(0) == 0).all() and (coords[:, :3].max(0) == 96).all() and 0 < keep.sum() < len(keep)
    if name == "coordinate_exactly_full_scale":
        assert keep.tolist() == [True, False, True, False, False, True] and coords[0, :3].tolist() == [0, 0, 0]
        assert coords[1, 0] == 64 and coords[2, :3].tolist() == [63, 63, 63]
    if name == "noisy_rotation":
        assert frac.min() > 1e-9 and 0 < keep.sum() and not np.array_equal(c["R"], np.eye(3)) and abs(np.linalg.det(c["R"])) > 0.5
    if name.startswith("flip"):
        assert np.array_equal(np.abs(c["R"]), np.eye(3)) and (np.diag(c["R"]) < 0).any()


def test_voxeliser_reference_reproduces_fixture_g8(golden_dir):
    """The restatement, fed G8's cloud, the oracle's occlusion culling and the reference's draws, gives G8's `locs_*` digests
    (the smallest of the three clouds)."""
    g8 = dict(np.load(os.path.join(golden_dir, "g8_vgi.npz")))
    k = int(np.argmin([int(g8[f"n_cat{i}"]) for i in range(3)]))
    locs, valid = vc.g8_post_process(k, g8)
    assert np.array_equal(np.packbits(valid), g8[f"pres_bits{k}"])
    assert len(locs) == int(g8[f"locs_n{k}"]) and np.array_equal(locs[:128], g8[f"locs_head{k}"])
    key = (locs[:, 0] << 24) | (locs[:, 1] << 12) | locs[:, 2]
    assert int(key.sum()) == int(g8[f"locs_keysum{k}"]) and int(np.bitwise_xor.reduce(key)) == int(g8[f"locs_keyxor{k}"])
