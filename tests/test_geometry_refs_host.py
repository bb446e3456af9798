"""The inputs and numpy references of tests/test_gpu_geometry_edges.py are what that file takes them for (no GPU needed):
a reference that is wrong, or an input that misses its edge, would otherwise make a device test pass for nothing."""
import numpy as np
import pytest

import _geometry_cases as gc
from oracle import scn3d
from oracle.voxelize import voxel_coords


# ------------------------------------------------------------------------------------------------ grouped rulebook
@pytest.mark.parametrize("K,A", gc.RB_SHAPES)
def test_grouped_rulebook_reference_is_the_table_as_a_multiset(K, A):
    nbr = gc.rb_table(K, A)
    tg, gs, go, gi, gout = gc.rb_reference(nbr)
    assert gc.rb_triples(gs, go, gi, gout) == gc.table_triples(nbr)
    # layout: offsets ascend inside a tile, lanes ascend inside a (tile, offset), padding only at the end of its last group
    assert gs[-1] == len(go) == tg.sum() <= gc.rb_group_bound(K, A)
    for t in range(len(tg)):
        o = go[gs[t]:gs[t + 1]]
        assert (np.diff(o) >= 0).all()
        for off in np.unique(o):
            lanes = gout[gs[t]:gs[t + 1]][o == off].reshape(-1)
            n = int((lanes >= 0).sum())
            assert (lanes[:n] >= 0).all() and (np.diff(lanes[:n]) > 0).all() and (lanes[n:] == -1).all() and len(lanes) - n < 16


def test_grouped_rulebook_reference_of_an_empty_table_and_by_hand():
    tg, gs, go, gi, gout = gc.rb_reference(np.full((27, 65), -1, np.int32))
    assert tg.tolist() == [0, 0] and gs.tolist() == [0, 0, 0] and go.size == 0 and gi.shape == (0, 16)
    # 17 rules of offset 1 in tile 0 (rows 3 .. 19), one rule of offset 0 in tile 1 (row 64)
    nbr = np.full((2, 65), -1, np.int32)
    nbr[1, 3:20] = np.arange(100, 117)
    nbr[0, 64] = 7
    tg, gs, go, gi, gout = gc.rb_reference(nbr)
    assert tg.tolist() == [2, 1] and gs.tolist() == [0, 2, 3] and go.tolist() == [1, 1, 0]
    assert gi[0].tolist() == list(range(100, 116)) and gout[0].tolist() == list(range(3, 19))
    assert gi[1].tolist() == [116] + [-1] * 15 and gout[1].tolist() == [19] + [-1] * 15
    assert gi[2].tolist() == [7] + [-1] * 15 and gout[2].tolist() == [0] + [-1] * 15


def test_synthetic_tables_hit_every_listed_rule_count():
    """0, 1, 15, 16, 17, 32, 33, 48, 49, 64 rules per (tile, offset): the 16/17, 32/33, 48/49 group boundaries and the full tile."""
    for K, A in gc.RB_SHAPES:
        hit = gc.rb_counts_hit(gc.rb_table(K, A))
        if K == 27 and A >= 64:
            assert hit >= set(gc.RB_COUNTS), (K, A, hit)
        if A == 1:
            assert hit == {0, 1}
        if A == 63:
            assert {15, 16, 17, 32, 33, 48, 49, 63} <= hit or K == 8
    assert set().union(*(gc.rb_counts_hit(gc.rb_table(8, A)) for A in (64, 65, 128, 129))) >= set(gc.RB_COUNTS)


# ------------------------------------------------------------------------------------------------ borders and the lattice
def _kernel_query_key(k, dx, dy, dz):
    """The key k_rulebook_subm would look up WITHOUT its range check: the fields ORed together after the step."""
    x, y, z = ((k >> 24) & 4095) + dx, ((k >> 12) & 4095) + dy, (k & 4095) + dz
    return (k & ~0xFFFFFFFFF) | (x << 24) | (y << 12) | z


@pytest.mark.parametrize("full_scale", [4096, 64])
def test_border_pairs_are_no_neighbours_in_the_oracle(full_scale):
    c, pairs = gc.border_cloud(full_scale)
    m = full_scale - 1
    assert c[:, :3].min() == 0 and c[:, :3].max() == m
    for ax in range(3):
        assert (c[:, ax] == 0).any() and (c[:, ax] == m).any()
    g = scn3d.Geometry(c, 3, full_scale)
    keys = scn3d.pack_keys(c).astype(np.int64)
    probed = []
    for i, j, (dx, dy, dz) in pairs:
        ri, rj = g.point_row[i], g.point_row[j]
        assert ri != rj and rj not in g.nbr27[0][:, ri] and ri not in g.nbr27[0][:, rj]
        if full_scale == 4096:   # ... and a kernel without the range check WOULD find j from i
            assert _kernel_query_key(int(keys[i]), dx, dy, dz) == int(keys[j])
        if (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1) <= 12:    # a step k_rulebook_subm makes itself (offsets 13 .. 26 are mirrored)
            probed.append((dx, dy, dz))
    assert any(dy == 1 for _, dy, _ in probed) and sum(dz == 1 for _, _, dz in probed) >= 2   # the y carry; the z carry both ways
    # the kernel's loop restated (13 probes, mirrored hits) gives the oracle's table; with its range test off by one it does not
    for l in range(3):
        assert np.array_equal(gc.subm_model(g.row_keys[l], full_scale >> l), g.nbr27[l])
    if full_scale == 4096:
        broken = gc.subm_model(g.row_keys[0], 4096, limit=4096)
        for i, j, step in pairs:
            if step in probed:
                assert g.point_row[j] in broken[:, g.point_row[i]] and g.point_row[i] in broken[:, g.point_row[j]]
    # the border voxels do have true neighbours, at every level, and the levels' last coordinate is reached: 63 / 31 / 15 at 64
    for l in range(3):
        xyz = scn3d.unpack_keys(g.row_keys[l])[:, :3]
        assert xyz.max() == (full_scale >> l) - 1 and xyz.min() == 0
        on_border = ((xyz == 0) | (xyz == (full_scale >> l) - 1)).any(1)
        nn = (g.nbr27[l] >= 0).sum(0)
        assert (nn[on_border] > 1).any() and (g.nbr27[l][:, on_border] == -1).any()


def test_oracle_geometry_refuses_voxels_outside_the_field():
    c = gc.cloud(3)
    scn3d.Geometry(c, 2, 64)
    c[5, 1] = 64
    with pytest.raises(AssertionError):
        scn3d.Geometry(c, 2, 64)
    scn3d.Geometry(c, 2, 4096)


def test_lattice_keys_share_their_in_block_position_and_wrap_the_table():
    for c in (gc.lattice(), gc.lattice_plus_block()):
        assert c[:, :3].min() == 0 and c[:, :3].max() == 60
    assert gc.dense_blocks()[:, :3].max() < 64
    c = gc.lattice()
    keys = scn3d.pack_keys(c)
    assert len(np.unique(keys)) == 4096 and (c[:, :3] % 4 == 0).all()
    cap = gc.pow2_at_least(2 * len(keys))
    assert cap == 8192                                   # load exactly 0.5
    home, local = gc.home_slot_model(keys, cap)
    assert (local == 0).all() and (home % 64 == 0).all() and len(np.unique(home)) <= cap // 64
    longest, crossed, wrapped = gc.probe_model(keys, cap)
    assert longest >= 32                                 # 32 keys per bucket on average, all on its first slot
    # the lattice alone never leaves a bucket (at most 47 keys per bucket in this model); the dense blocks do, and wrap
    keys = scn3d.pack_keys(gc.dense_blocks())
    assert len(np.unique(keys)) == 4096 and gc.pow2_at_least(2 * len(keys)) == 8192
    longest, crossed, wrapped = gc.probe_model(keys, 8192)
    assert longest >= 64 and crossed > 0                 # chains longer than a bucket, running over bucket ends
    assert wrapped > 0                                   # ... and over the end of the table: the `& mask` of the probe loops
    assert gc.probe_model(keys, 8 * 8192)[2] == 0        # the 8-fold table does not wrap: the two runs probe differently
    # the coarse levels of the lattice: stride 2, then the dense 16^3 block
    g = scn3d.Geometry(c, 3, 64)
    assert g.num_active == [4096, 4096, 4096] and (g.nbr27[0] >= 0).sum() == 4096 and (g.nbr27[2] >= 0).sum(0).max() == 27
    gb = scn3d.Geometry(gc.lattice_plus_block(), 3, 64)
    assert gb.num_active[0] == 4096 + 216 - 1 and (gb.nbr27[0] >= 0).sum(0).max() == 27


# ------------------------------------------------------------------------------------------------ the other references
def test_scan_inputs_and_reference():
    assert gc.scan_reference(np.asarray([3, 0, 5], np.int32))[0].tolist() == [0, 3, 3] and gc.scan_reference(np.asarray([3, 0, 5], np.int32))[1] == 8
    for n in (8192, 8193, 262144, 262145):
        assert n in gc.SCAN_SIZES
    v = gc.scan_input(300001, "counts")
    assert v.max() == 500 and v.min() == 0 and gc.scan_reference(v)[1] < 2 ** 31
    assert set(np.unique(gc.scan_input(1025, "flags")).tolist()) == {0, 1}
    # every 256-block trip of the sums kernel carries something in: the first 262144 items are not all zero
    assert gc.scan_reference(gc.scan_input(262145, "flags")[:262144])[1] > 0


def test_stride2_cases_are_what_their_names_say():
    cases = gc.stride2_cases()
    g = scn3d.Geometry(cases["all_8_children"], 2, 4096)
    assert g.num_active == [8, 1] and sorted(g.ch[0][:, 0].tolist()) == list(range(8))
    g = scn3d.Geometry(cases["one_child_per_octant"], 2, 4096)
    assert g.num_active == [9, 9] and ((g.ch[0] >= 0).sum(0) == 1).all() and ((g.ch[0][:, :8] >= 0).sum(1) == 1).all()
    g = scn3d.Geometry(cases["all_8_and_single_children"], 2, 4096)
    assert sorted((g.ch[0] >= 0).sum(0).tolist()) == [1] * 8 + [8]
    g = scn3d.Geometry(cases["num_coarse_1"], 2, 4096)
    assert g.num_active == [3, 1]


def test_csr_cases_and_reference():
    cases = gc.csr_cases()
    pr, A = cases["one_row_holds_3000_of_3500"]
    assert len(pr) == 3500 and np.bincount(pr, minlength=A).max() >= 3000
    pr, A = cases["20000_points_9000_rows"]
    assert A > 8192 and pr.max() < A
    pr, A = cases["5000_points_12000_rows_mostly_empty"]
    cnt = np.bincount(pr, minlength=A)
    assert A == 12000 and cnt[0] == 0 and cnt[-1] == 0 and (cnt == 0).sum() > A // 2
    rs, rp = gc.csr_reference(np.asarray([2, 0, 2, 2, 0], np.int32), 4)
    assert rs.tolist() == [0, 2, 2, 5, 5] and rp.tolist() == [1, 4, 0, 2, 3]


def test_coarsen_reference_against_the_oracle_geometry():
    keys = gc.distinct_keys(5000, 1)
    assert len(np.unique(keys)) == 5000
    g = scn3d.Geometry(scn3d.unpack_keys(keys), 2, 4096)
    ck, parent = gc.coarsen_reference(keys)
    assert np.array_equal(ck, g.row_keys[1]) and np.array_equal(parent, g.parent[0]) and len(ck) < 5000


def test_voxel_cases_reach_their_edges():
    cases = gc.voxel_cases()
    pts, scale, fs, u = cases["ties_to_even"]
    v = pts.astype(np.float64) * scale
    assert (v - np.floor(v) == 0.5).all() and (v < 0).any() and (v > 0).any()
    assert (np.round(v) % 2 == 0).all()
    pts, scale, fs, u = cases["span_u_just_below_1"]
    assert all(0 < x < 1 for x in u)
    r = np.round(pts * np.float32(scale))
    t = np.float32(fs) - (r - r.min(0)).max(0) - np.float32(0.001)
    assert t[0] < 0 and 0 < t[1] < 1 and t[2] > 1           # the clip to 0 engages in axis 0 only
    for name in ("span_u0", "wider_than_the_field", "wider_than_the_field_translated"):
        pts, scale, fs, u = cases[name]
        ci, keep = voxel_coords(pts, scale, fs, u)
        assert 0 < keep.sum() < len(keep), name
    for pts, scale, fs, u in cases.values():
        assert np.isfinite(pts).all()
