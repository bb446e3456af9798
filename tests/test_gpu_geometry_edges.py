"""The integer geometry build, entry point by entry point, at its edges.  Run with -m gpu on an MI355X.

Every test calls the C ABI directly (mopa_amd._lib: call / query / ptr / stream) and compares with numpy in int64 or with the
integer part of oracle/scn3d.py / oracle/voxelize.py: equalities only.  Output buffers are larger than the contract needs and
pre-filled with a sentinel; what the contract does not cover must still hold it afterwards.  Workspaces are exactly as large as
the *_workspace_bytes query says, with a guard behind them.  Inputs and references: tests/_geometry_cases.py (checked on the
host by tests/test_geometry_refs_host.py).
"""
import numpy as np
import pytest
import torch

import _geometry_cases as gc
from oracle import scn3d
from oracle.voxelize import voxel_coords

pytestmark = pytest.mark.gpu

SENT = -1515870811                      # 0xA5A5A5A5 as int32: no row number, count or -1 padding looks like it
SENT64 = 0x5A5A5A5A5A5A5A5A             # no key looks like it (x, y, z <= 4095 here would need batch 0x5A5A5A5)
PAD = 64


def _L():
    from mopa_amd import _lib
    return _lib


def _buf(n, dtype=torch.int32, pad=PAD):
    """n + pad elements on the device, all of them the sentinel."""
    return torch.full((n + pad,), SENT64 if dtype == torch.int64 else SENT, dtype=dtype, device="cuda")


def _untouched(t, n=0):
    """The elements of a _buf behind the first n still hold the sentinel."""
    return bool((t[n:] == (SENT64 if t.dtype == torch.int64 else SENT)).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Ws:
    """A workspace of exactly the queried size; `ok()` = nothing was written behind it."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.t = torch.full((self.nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")

    def ok(self):
        return bool((self.t[self.nbytes:] == 0xA5).all())


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------------------------ exclusive scan
def _scan(v, n=None, ws_short=0):
    L = _L()
    n = len(v) if n is None else n
    x, out, total = _dev(v), _buf(len(v)), _buf(1)
    ws = _Ws(L.query("mopa_scan_workspace_bytes", max(n, 1)))
    L.call("mopa_scan_exclusive_i32", L.ptr(x), L.ptr(out), n, L.ptr(total), L.ptr(ws.t), ws.nbytes - ws_short, L.stream())
    return out, total, ws


@pytest.mark.parametrize("n", gc.SCAN_SIZES)
def test_scan_exclusive_equals_cumsum(n):
    """One block up to 8192, three launches from 8193, a second 256-block trip of the sums kernel from 262145; flags and counts."""
    for kind in gc.SCAN_KINDS:
        v = gc.scan_input(n, kind)
        ref, ref_total = gc.scan_reference(v)
        out, total, ws = _scan(v)
        assert np.array_equal(out[:n].cpu().numpy().astype(np.int64), ref), (n, kind)
        assert int(total[0]) == ref_total, (n, kind)
        assert _untouched(out, n) and _untouched(total, 1) and ws.ok(), (n, kind)


@pytest.mark.parametrize("n", [5, 8193, 262145])
def test_scan_refuses_a_short_workspace_and_an_empty_input(n):
    v = gc.scan_input(n, "counts")
    L = _L()
    x, out, total = _dev(v), _buf(n), _buf(1)
    wsb = L.query("mopa_scan_workspace_bytes", n)
    ws = _Ws(wsb)
    with pytest.raises(RuntimeError):
        L.call("mopa_scan_exclusive_i32", L.ptr(x), L.ptr(out), n, L.ptr(total), L.ptr(ws.t), wsb - 1, L.stream())
    with pytest.raises(RuntimeError):
        L.call("mopa_scan_exclusive_i32", L.ptr(x), L.ptr(out), 0, L.ptr(total), L.ptr(ws.t), wsb, L.stream())
    torch.cuda.synchronize()
    assert _untouched(out) and _untouched(total) and bool((ws.t == 0xA5).all())


# ------------------------------------------------------------------------------------------------ level 0: first-seen unique
def _hash_build(coords, cap=None, pad=PAD):
    """mopa_voxel_hash_build on coords (N,4) int64 -> dict of device buffers (sentinel-padded) + the workspace guard."""
    L = _L()
    N = len(coords)
    cap = gc.pow2_at_least(2 * N) if cap is None else cap
    r = dict(N=N, cap=cap, coords=_dev(coords), tk=_buf(cap, torch.int64), tv=_buf(cap), point_row=_buf(N), row_keys=_buf(N, torch.int64),
             num_rows=_buf(1), status=torch.zeros(1 + pad, dtype=torch.int32, device="cuda"),
             ws=_Ws(L.query("mopa_voxel_hash_workspace_bytes", N)))
    L.call("mopa_voxel_hash_build", L.ptr(r["coords"]), N, L.ptr(r["tk"]), L.ptr(r["tv"]), cap, L.ptr(r["point_row"]), L.ptr(r["row_keys"]),
           L.ptr(r["num_rows"]), L.ptr(r["status"]), L.ptr(r["ws"].t), r["ws"].nbytes, L.stream())
    return r


def _check_level0(r, coords):
    keys = scn3d.pack_keys(coords)
    ref_keys, ref_row = scn3d.first_seen_unique(keys)
    N, A = r["N"], len(ref_keys)
    assert int(r["num_rows"][0]) == A and int(r["status"][0]) == 0
    assert np.array_equal(r["point_row"][:N].cpu().numpy(), ref_row.astype(np.int32))
    assert np.array_equal(_u64(r["row_keys"][:A]), ref_keys)
    assert _untouched(r["point_row"], N) and _untouched(r["row_keys"], A) and _untouched(r["num_rows"], 1)
    assert _untouched(r["tk"], r["cap"]) and _untouched(r["tv"], r["cap"]) and r["ws"].ok() and not bool(r["status"][1:].any())
    # the table is an index of exactly these rows
    tk, tv = _u64(r["tk"][:r["cap"]]), r["tv"][:r["cap"]].cpu().numpy()
    used = tk != np.uint64(0xFFFFFFFFFFFFFFFF)
    assert used.sum() == A and np.array_equal(ref_keys[tv[used]], tk[used])
    return A


def _distinct_coords(n, seed, box=41, batches=3):
    return scn3d.unpack_keys(gc.distinct_keys(n, seed, box, batches))


def test_hash_build_one_point_and_one_voxel():
    _check_level0(_hash_build(np.asarray([[4095, 0, 4095, 5]], np.int64)), np.asarray([[4095, 0, 4095, 5]], np.int64))
    c = np.tile(np.asarray([[17, 4095, 0, 2]], np.int64), (1000, 1))      # all points in one voxel
    assert _check_level0(_hash_build(c), c) == 1


@pytest.mark.parametrize("n", [4096, 8193])
def test_hash_build_all_points_distinct(n):
    """N = 4096: table_cap = pow2(2 N) = 8192 sits at load exactly 0.5.  N = 8193: the three-launch scan, every flag set."""
    c = _distinct_coords(n, 2)
    r = _hash_build(c)
    assert r["cap"] == (8192 if n == 4096 else 32768)
    assert _check_level0(r, c) == n
    if n == 4096:   # ... the lattice, whose keys all want slot 0 of their bucket, and the blocks that wrap the table: same load
        for c in (gc.lattice(), gc.dense_blocks()):
            r = _hash_build(c)
            assert r["cap"] == 8192 and _check_level0(r, c) == 4096


def test_hash_build_262145_points_heavy_duplication():
    """Past 256 scan blocks (n > 262144) with an oracle: ~5000 voxels, every one hit ~50 times -- and 1000 voxels first seen in
    the last 1000 points, so that the row numbers behind the 256th block depend on everything in front of it."""
    rng = np.random.Generator(np.random.PCG64(3))
    vox = _distinct_coords(6000, 4)
    c = np.concatenate([vox[rng.integers(0, 5000, 262145 - 1000)], vox[5000:]])
    assert 5000 < _check_level0(_hash_build(c), c) <= 6000


def test_hash_build_batch_indices_up_to_2_pow_27():
    """The same x, y, z in different batches are different voxels; batch 2^27 - 1 is the last one a key can hold."""
    rng = np.random.Generator(np.random.PCG64(6))
    xyz = rng.integers(0, 4096, (50, 3))
    batches = np.asarray([0, 1, 2, 2 ** 26, 2 ** 27 - 2, 2 ** 27 - 1], np.int64)
    c = np.concatenate([np.concatenate([xyz, np.full((50, 1), b)], 1) for b in batches]).astype(np.int64)
    c = c[rng.integers(0, len(c), 2000)]
    A = _check_level0(_hash_build(c), c)
    assert A == len(np.unique(c, axis=0)) > 250


@pytest.mark.parametrize("col,value", [(0, 4096), (1, 4096), (2, 4096), (0, -1), (2, -4096), (3, 2 ** 27), (3, -1)])
def test_hash_build_status_bit_for_a_coordinate_out_of_range(col, value):
    c = gc.cloud(3)
    assert int(_hash_build(c)["status"][0]) == 0
    c[1234, col] = value
    r = _hash_build(c)
    assert int(r["status"][0]) == 1 and not bool(r["status"][1:].any())
    assert _untouched(r["point_row"], r["N"]) and _untouched(r["tk"], r["cap"]) and r["ws"].ok()


def test_hash_build_and_coarsen_refuse_a_bad_table_capacity():
    L = _L()
    c = _distinct_coords(1000, 7)
    for cap in (1024, 3000, 2047, 0):          # below 2 N (a power of two), not a power of two (above 2 N and below), none
        with pytest.raises(RuntimeError):
            _hash_build(c, cap=cap)
    r = _hash_build(c, cap=2048)
    _check_level0(r, c)
    N = 1000
    for cap in (1024, 3000):
        parent, ck, nc = _buf(N), _buf(N, torch.int64), _buf(1)
        tk, tv = _buf(4096, torch.int64), _buf(4096)
        ws = _Ws(L.query("mopa_coarsen_workspace_bytes", N))
        with pytest.raises(RuntimeError):
            L.call("mopa_coarsen_build", L.ptr(r["row_keys"]), N, L.ptr(r["num_rows"]), L.ptr(tk), L.ptr(tv), cap, L.ptr(parent), L.ptr(ck),
                   L.ptr(nc), L.ptr(ws.t), ws.nbytes, L.stream())
        torch.cuda.synchronize()
        assert _untouched(parent) and _untouched(ck) and _untouched(nc) and _untouched(tk) and _untouched(tv) and ws.ok()
    ws = _Ws(L.query("mopa_voxel_hash_workspace_bytes", N))
    pr = _buf(N)
    with pytest.raises(RuntimeError):          # a workspace one byte short
        L.call("mopa_voxel_hash_build", L.ptr(r["coords"]), N, L.ptr(r["tk"]), L.ptr(r["tv"]), 2048, L.ptr(pr), L.ptr(r["row_keys"]),
               L.ptr(r["num_rows"]), L.ptr(r["status"]), L.ptr(ws.t), ws.nbytes - 1, L.stream())
    torch.cuda.synchronize()
    assert _untouched(pr) and bool((ws.t == 0xA5).all())


# ------------------------------------------------------------------------------------------------ coarsening
def _coarsen(fine_keys_dev, n_cap, count_dev, cap):
    """mopa_coarsen_build with the count on the device -> (parent, coarse_keys, num_coarse, tk, tv, ws)."""
    L = _L()
    parent, ck, nc = _buf(n_cap), _buf(n_cap, torch.int64), _buf(1)
    tk, tv = _buf(cap, torch.int64), _buf(cap)
    ws = _Ws(L.query("mopa_coarsen_workspace_bytes", n_cap))
    L.call("mopa_coarsen_build", L.ptr(fine_keys_dev), n_cap, L.ptr(count_dev), L.ptr(tk), L.ptr(tv), cap, L.ptr(parent), L.ptr(ck), L.ptr(nc),
           L.ptr(ws.t), ws.nbytes, L.stream())
    return parent, ck, nc, tk, tv, ws


@pytest.mark.parametrize("count,cap", [(5000, 9000), (8193, 20000), (20000, 20000), (100, 262145)])
def test_coarsen_build_with_a_device_count_below_the_capacity(count, cap):
    """The count is read on the device; the capacity picks the scan (one block <= 8192 < three launches, two trips > 262144)."""
    keys = gc.distinct_keys(count, 8)
    ref_ck, ref_parent = gc.coarsen_reference(keys)
    fine = torch.full((cap,), 0x0000001000FFFFFF, dtype=torch.int64, device="cuda")   # behind the count: a real-looking key of batch 1
    fine[:count] = _dev(keys.view(np.int64))
    parent, ck, nc, tk, tv, ws = _coarsen(fine, cap, torch.tensor([count], dtype=torch.int32, device="cuda"), gc.pow2_at_least(2 * cap))
    C = len(ref_ck)
    assert int(nc[0]) == C
    assert np.array_equal(parent[:count].cpu().numpy(), ref_parent) and np.array_equal(_u64(ck[:C]), ref_ck)
    assert _untouched(parent, count) and _untouched(ck, C) and _untouched(nc, 1)
    assert _untouched(tk, gc.pow2_at_least(2 * cap)) and _untouched(tv, gc.pow2_at_least(2 * cap)) and ws.ok()


# ------------------------------------------------------------------------------------------------ the whole chain
def _chain(coords, levels, full_scale, cap_mult=1):
    """Level 0, levels - 1 coarsenings (counts stay on the device), then mopa_rulebook_subm per level and mopa_rulebook_updown
    between levels, at table_cap = pow2(2 N) * cap_mult.  -> dict of numpy arrays named like oracle.scn3d.Geometry's fields."""
    L = _L()
    N = len(coords)
    cap = gc.pow2_at_least(2 * N) * cap_mult
    r = _hash_build(coords, cap=cap)
    assert int(r["status"][0]) == 0
    keys, tks, tvs, counts, parents = [r["row_keys"]], [r["tk"]], [r["tv"]], [r["num_rows"]], []
    for l in range(levels - 1):
        parent, ck, nc, tk, tv, ws = _coarsen(keys[l], N, counts[l], cap)
        keys.append(ck), tks.append(tk), tvs.append(tv), counts.append(nc), parents.append(parent)
        assert ws.ok()
    A = [int(c[0]) for c in counts]
    out = dict(num_active=A, point_row=r["point_row"][:N].cpu().numpy(), row_keys=[_u64(keys[l][:A[l]]) for l in range(levels)],
               parent=[parents[l][:A[l]].cpu().numpy() for l in range(levels - 1)], nbr27=[], ch=[], up=[])
    for l in range(levels):
        assert _untouched(keys[l], A[l]) and _untouched(tks[l], cap) and _untouched(tvs[l], cap)
        if l:
            assert _untouched(parents[l - 1], A[l - 1])
        nbr = _buf(27 * A[l])
        L.call("mopa_rulebook_subm", L.ptr(keys[l]), A[l], L.ptr(tks[l]), L.ptr(tvs[l]), cap, full_scale >> l, L.ptr(nbr), L.stream())
        assert _untouched(nbr, 27 * A[l])
        out["nbr27"].append(nbr[:27 * A[l]].cpu().numpy().reshape(27, A[l]))
    for l in range(levels - 1):
        ch, up = _buf(8 * A[l + 1]), _buf(8 * A[l])
        L.call("mopa_rulebook_updown", L.ptr(keys[l]), L.ptr(parents[l]), A[l], A[l + 1], L.ptr(ch), L.ptr(up), L.stream())
        assert _untouched(ch, 8 * A[l + 1]) and _untouched(up, 8 * A[l])
        out["ch"].append(ch[:8 * A[l + 1]].cpu().numpy().reshape(8, A[l + 1]))
        out["up"].append(up[:8 * A[l]].cpu().numpy().reshape(8, A[l]))
    return out


def _assert_chain_equals_oracle(got, o):
    assert got["num_active"] == o.num_active
    assert np.array_equal(got["point_row"], o.point_row)
    for l in range(o.num_levels):
        assert np.array_equal(got["row_keys"][l], o.row_keys[l]), l
        assert np.array_equal(got["nbr27"][l], o.nbr27[l]), l
    for l in range(o.num_levels - 1):
        assert np.array_equal(got["parent"][l], o.parent[l]), l
        assert np.array_equal(got["ch"][l], o.ch[l]), l
        assert np.array_equal(got["up"][l], o.up[l]), l


@pytest.mark.parametrize("name", ["lattice", "lattice_plus_block", "dense_blocks", "cloud"])
def test_results_do_not_depend_on_the_hash_table(name):
    """table_cap = pow2(2 N) and 8 times that: same rows, same rule tables, both equal to the oracle.  The lattice (4096 voxels
    of stride 4 at load exactly 0.5) puts every key on slot 0 of its bucket; the dense blocks (64 full 4x4x4 blocks, same load)
    overfill buckets: probe chains over bucket ends and over the end of the table, where `& mask` wraps them to slot 0."""
    coords = dict(lattice=gc.lattice, lattice_plus_block=gc.lattice_plus_block, dense_blocks=gc.dense_blocks, cloud=lambda: gc.cloud(0))[name]()
    o = scn3d.Geometry(coords, 3, 64)
    small, large = _chain(coords, 3, 64, 1), _chain(coords, 3, 64, 8)
    _assert_chain_equals_oracle(small, o)
    _assert_chain_equals_oracle(large, o)


@pytest.mark.parametrize("full_scale", [4096, 64])
def test_borders_and_field_carry(full_scale):
    """Voxels at 0 and at full_scale - 1 of every axis (63 / 31 / 15 at the three levels of full_scale = 64).  At 4096, x + 1 of
    (4095, y, z, 0) would carry into the batch field and find (0, y, z, 1), y + 1 of (x, 4095, z, 0) into x and find (x + 1, 0, z, 0),
    z + 1 of (x, y, 4095, 0) into y and find (x, y + 1, 0, 0): only the range check of k_rulebook_subm keeps them apart.  The
    kernel makes the +y / +z steps together with dx = -1 or dy = -1 (offsets 0 .. 12); the cloud holds pairs for those too."""
    coords, pairs = gc.border_cloud(full_scale)
    o = scn3d.Geometry(coords, 3, full_scale)
    got = _chain(coords, 3, full_scale)
    _assert_chain_equals_oracle(got, o)
    for i, j, _ in pairs:
        ri, rj = got["point_row"][i], got["point_row"][j]
        assert rj not in got["nbr27"][0][:, ri] and ri not in got["nbr27"][0][:, rj], (i, j)


@pytest.mark.parametrize("name", list(gc.stride2_cases()))
def test_stride2_tables(name):
    """A coarse voxel with all 8 children, coarse voxels with exactly one child in each octant, num_coarse = 1."""
    coords = gc.stride2_cases()[name]
    o = scn3d.Geometry(coords, 2, 4096)
    got = _chain(coords, 2, 4096)
    _assert_chain_equals_oracle(got, o)
    if name == "num_coarse_1":
        assert got["num_active"][1] == 1


# ------------------------------------------------------------------------------------------------ point CSR
@pytest.mark.parametrize("name", list(gc.csr_cases()))
def test_points_csr_whole_arrays(name):
    """row_start and row_points in full against a stable argsort: one row of 3000 points (the insertion sort repairs the order
    the atomics left), 9000 and 12000 rows (the three-launch scan), empty rows -- the first and the last included."""
    L = _L()
    point_row, A = gc.csr_cases()[name]
    N = len(point_row)
    ref_start, ref_points = gc.csr_reference(point_row, A)
    pr, rs, rp = _dev(point_row), _buf(A + 1), _buf(N)
    ws = _Ws(L.query("mopa_points_csr_workspace_bytes", A))
    L.call("mopa_points_csr", L.ptr(pr), N, A, L.ptr(rs), L.ptr(rp), L.ptr(ws.t), ws.nbytes, L.stream())
    assert np.array_equal(rs[:A + 1].cpu().numpy(), ref_start)
    assert np.array_equal(rp[:N].cpu().numpy(), ref_points)
    assert _untouched(rs, A + 1) and _untouched(rp, N) and ws.ok()
    with pytest.raises(RuntimeError):
        L.call("mopa_points_csr", L.ptr(pr), N, A, L.ptr(rs), L.ptr(rp), L.ptr(ws.t), ws.nbytes - 1, L.stream())


# ------------------------------------------------------------------------------------------------ group split
def _group_split(item_row_dev, n_cap, n_host=0, n_dev=None):
    L = _L()
    out = _buf(1)
    out[0] = 0                                   # the contract: out[0] is 0 before
    L.call("mopa_group_split", L.ptr(item_row_dev), None if n_dev is None else L.ptr(n_dev), n_host, n_cap, L.ptr(out), L.stream())
    assert _untouched(out, 1)
    return int(out[0])


@pytest.mark.parametrize("n_cap,count", [(10, 1), (257, 256), (5000, 3000), (300000, 299999), (1_048_579, 1_048_576)])
def test_group_split_counts_on_the_host_and_on_the_device(n_cap, count):
    """out = max(item_row[:count]) + 1.  The maximum sits in the LAST counted element; everything behind the count is larger and
    must be ignored.  n_cap = 1,048,579 is past the 512-block grid cap (a grid-stride loop of 8+ items per thread)."""
    rng = np.random.Generator(np.random.PCG64(n_cap))
    v = rng.integers(0, 1000, n_cap).astype(np.int32)
    v[count - 1] = 4321
    v[count:] = 1_000_000
    x = _dev(v)
    assert _group_split(x, n_cap, n_host=0) == 0                                            # nothing counted: the output stays 0
    host = _group_split(x, n_cap, n_host=count)
    dev = _group_split(x, n_cap, n_host=0, n_dev=torch.tensor([count], dtype=torch.int32, device="cuda"))
    assert host == dev == 4322 == int(v[:count].astype(np.int64).max()) + 1
    assert _group_split(x, n_cap, n_host=count - 1) == (int(v[:count - 1].max()) + 1 if count > 1 else 0)
    assert _group_split(x, n_cap, n_host=n_cap) == 1_000_001
    with pytest.raises(RuntimeError):
        _group_split(x, n_cap, n_host=n_cap + 1)


# ------------------------------------------------------------------------------------------------ grouped rulebook
def _rb_arrays(total_bound):
    return _buf(total_bound), _buf(total_bound * 16), _buf(total_bound * 16)


def _assert_rulebook(go, gi, gout, g0, ref):
    """The groups g0 .. g0 + G - 1 of the shared arrays equal the reference of one table."""
    _, _, r_go, r_gi, r_gout = ref
    G = len(r_go)
    assert np.array_equal(go[g0:g0 + G].cpu().numpy(), r_go)
    assert np.array_equal(gi[16 * g0:16 * (g0 + G)].cpu().numpy().reshape(G, 16), r_gi)
    assert np.array_equal(gout[16 * g0:16 * (g0 + G)].cpu().numpy().reshape(G, 16), r_gout)


def _rb_single(nbr):
    """mopa_rulebook_groups_count + mopa_rulebook_groups_fill on one table, checked against the reference."""
    L = _L()
    K, A = nbr.shape
    ref = gc.rb_reference(nbr)
    tiles, bound = (A + 63) // 64, gc.rb_group_bound(K, A)
    t, tg = _dev(nbr), _buf(tiles)
    L.call("mopa_rulebook_groups_count", L.ptr(t), K, A, L.ptr(tg), L.stream())
    assert np.array_equal(tg[:tiles].cpu().numpy(), ref[0]) and _untouched(tg, tiles)
    G = int(ref[1][-1])
    assert G <= bound                              # what Geometry3D sizes the arrays from
    gs = _dev(ref[1][:tiles].astype(np.int32))
    go, gi, gout = _rb_arrays(bound)
    L.call("mopa_rulebook_groups_fill", L.ptr(t), K, A, L.ptr(gs), L.ptr(go), L.ptr(gi), L.ptr(gout), L.stream())
    _assert_rulebook(go, gi, gout, 0, ref)
    assert _untouched(go, G) and _untouched(gi, 16 * G) and _untouched(gout, 16 * G)
    return ref


@pytest.mark.parametrize("K,A", gc.RB_SHAPES)
def test_grouped_rulebook_single_table_exact_layout(K, A):
    """Tables of 1, 63, 64, 65, 128, 129 rows with 0, 1, 15, 16, 17, 32, 33, 48, 49, 64 rules per (tile, offset): ceil(n / 16)
    groups at n = 16 / 17, 32 / 33, 48 / 49, 64 -- groups by offset inside a tile, rules by lane rank inside a group, -1 padding."""
    _rb_single(gc.rb_table(K, A))


def test_grouped_rulebook_all_minus_one_table():
    ref = _rb_single(np.full((27, 129), -1, np.int32))
    assert ref[1][-1] == 0


@pytest.mark.parametrize("shapes", [[(27, 129), (8, 65), (27, 63)], [(8, 1), (27, 64), (8, 128)], [(27, 65), None, (8, 129)]])
def test_grouped_rulebook_batched_equals_the_single_calls(shapes):
    """Three tables in one count launch, one device scan, one fill launch: table by table the single-table layout, at the
    table's slice of the global group numbering.  None = an all -1 table (27 x 70) between two others."""
    L = _L()
    tabs = [np.full((27, 70), -1, np.int32) if s is None else gc.rb_table(*s, seed=i) for i, s in enumerate(shapes)]
    refs = [gc.rb_reference(t) for t in tabs]
    dev = [_dev(t) for t in tabs]
    tile0 = np.concatenate([[0], np.cumsum([(t.shape[1] + 63) // 64 for t in tabs])])
    ntile = int(tile0[-1])
    desc = np.asarray([[d.data_ptr(), t.shape[0], t.shape[1], tile0[i]] for i, (d, t) in enumerate(zip(dev, tabs))], np.int64)
    tg, gs = _buf(ntile), _buf(ntile + 1)
    L.call("mopa_rulebook_groups_count_batched", desc.ctypes.data, len(tabs), ntile, L.ptr(tg), L.stream())
    ws = _Ws(L.query("mopa_scan_workspace_bytes", ntile))
    L.call("mopa_scan_exclusive_i32", L.ptr(tg), L.ptr(gs), ntile, L.ptr(gs, ntile), L.ptr(ws.t), ws.nbytes, L.stream())
    ref_tg = np.concatenate([r[0] for r in refs])
    ref_gs = np.concatenate([[0], np.cumsum(ref_tg)])
    assert np.array_equal(tg[:ntile].cpu().numpy(), ref_tg) and np.array_equal(gs[:ntile + 1].cpu().numpy(), ref_gs)
    assert _untouched(tg, ntile) and _untouched(gs, ntile + 1) and ws.ok()
    bound = sum(gc.rb_group_bound(*t.shape) for t in tabs)
    G = int(ref_gs[-1])
    assert G <= bound
    go, gi, gout = _rb_arrays(bound)
    L.call("mopa_rulebook_groups_fill_batched", desc.ctypes.data, len(tabs), ntile, L.ptr(gs), L.ptr(go), L.ptr(gi), L.ptr(gout), L.stream())
    for i, r in enumerate(refs):
        _assert_rulebook(go, gi, gout, int(ref_gs[tile0[i]]), r)
    assert _untouched(go, G) and _untouched(gi, 16 * G) and _untouched(gout, 16 * G)
    for n in (0, 33):                                   # no table, more tables than a launch takes
        with pytest.raises(RuntimeError):
            L.call("mopa_rulebook_groups_count_batched", desc.ctypes.data, n, ntile, L.ptr(tg), L.stream())


# ------------------------------------------------------------------------------------------------ voxeliser
@pytest.mark.parametrize("name", list(gc.voxel_cases()))
def test_voxelize_scan_equals_the_oracle(name):
    """Coordinates and keep: a single point, scaled values of exactly k + 0.5 (ties to even, k < 0 and k > 0), translation draws
    u = 0 and u = 1 - 2^-53 on a cloud that spans the field (the clip of the free room to 0 engages), clouds wider than the field."""
    from mopa_amd.voxelize import voxelize_scan
    pts, scale, fs, u = gc.voxel_cases()[name]
    ci, keep = voxel_coords(pts, scale, fs, u)
    coords, k = voxelize_scan(_dev(pts), scale, fs, u, batch_index=3)
    assert np.array_equal(k.cpu().numpy(), keep)
    want = np.concatenate([ci[keep], np.full((int(keep.sum()), 1), 3, np.int64)], 1)
    assert np.array_equal(coords.cpu().numpy(), want)
