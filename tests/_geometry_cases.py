"""Inputs and numpy references of the geometry-build edge tests (tests/test_gpu_geometry_edges.py runs them on the device,
tests/test_geometry_refs_host.py checks that the inputs are what the device tests take them for and that the references
restate what they claim to).  No GPU, no torch: numpy in int64 and the integer part of oracle/scn3d.py.
"""
import numpy as np

from oracle import scn3d

# ------------------------------------------------------------------------------------------------ exclusive scan
# csrc/hash3d.hip: one block for n <= 8192, three launches above, a second 256-block trip of the sums kernel for n > 262144
SCAN_SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4097, 8191, 8192, 8193, 9217, 262144, 262145, 300001]
SCAN_KINDS = ["zeros", "ones", "flags", "counts"]


def scan_input(n, kind, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed + n))
    if kind == "zeros":
        return np.zeros(n, np.int32)
    if kind == "ones":
        return np.ones(n, np.int32)
    if kind == "flags":
        return rng.integers(0, 2, n).astype(np.int32)
    return rng.integers(0, 501, n).astype(np.int32)   # group counts per tile: 300001 * 500 < 2^31


def scan_reference(v):
    """-> (exclusive prefix sums, total), summed in int64."""
    c = np.cumsum(v.astype(np.int64))
    return (c - v).astype(np.int64), int(c[-1])


def pow2_at_least(n):
    p = 1
    while p < n:
        p <<= 1
    return p


# ------------------------------------------------------------------------------------------------ point clouds
def cloud(seed, n=3000, size=48, batch=3):
    """The clustered cloud of tests/test_gpu_3d.py: non-trivial neighbourhoods, duplicate points."""
    rng = np.random.Generator(np.random.PCG64(seed))
    centers = rng.integers(4, size - 4, (40, 3))
    c = centers[rng.integers(0, 40, n)] + rng.integers(-3, 4, (n, 3))
    c = np.clip(c, 0, size - 1)
    b = rng.integers(0, batch, (n, 1))
    return np.concatenate([c, b], 1).astype(np.int64)


def lattice(seed=0):
    """4096 voxels on a 16^3 lattice of stride 4, in a shuffled order: every coordinate is a multiple of 4, so every key has
    in-block position 0 and wants slot 0 of its 64-slot bucket.  At table_cap = pow2(2 * 4096) = 8192 (load 0.5) that is 4096 keys
    on 128 home slots: probe chains of 30 - 50 slots.  (They stay inside their buckets -- no bucket gets more than 64 keys; for
    chains over bucket ends and over the end of the table see dense_blocks.)"""
    g = np.arange(16) * 4
    c = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    c = c[np.random.Generator(np.random.PCG64(seed)).permutation(len(c))]
    return np.concatenate([c, np.zeros((len(c), 1), np.int64)], 1).astype(np.int64)


def lattice_plus_block(seed=0):
    """The lattice and a dense 6^3 block (coordinates 17 .. 22: 27 neighbours everywhere inside, one lattice voxel in it twice)."""
    g = np.arange(17, 23)
    blk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    blk = np.concatenate([blk, np.zeros((len(blk), 1), np.int64)], 1).astype(np.int64)
    c = np.concatenate([lattice(seed), blk])
    return c[np.random.Generator(np.random.PCG64(seed + 1)).permutation(len(c))]


DENSE_BLOCKS_SEED = 9


def dense_blocks(seed=DENSE_BLOCKS_SEED, blocks=64):
    """`blocks` full 4x4x4 blocks of voxels (64 keys that fill one 64-slot bucket each) at random block positions of a 64^3
    field, shuffled: 4096 voxels at table_cap = 8192 are 64 full buckets' worth on 128 buckets, so two blocks that share a bucket
    spill over the bucket's end into the next ones.  The seed is chosen (test_geometry_refs_host.py checks it against a model of
    the hash) so that a chain also runs over the END OF THE TABLE and wraps to slot 0."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lin = rng.choice(16 ** 3, blocks, replace=False)
    org = np.stack([lin % 16, (lin // 16) % 16, lin // 256], 1) * 4
    g = np.arange(4)
    cell = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    c = (org[:, None, :] + cell[None]).reshape(-1, 3)
    c = c[rng.permutation(len(c))]
    return np.concatenate([c, np.zeros((len(c), 1), np.int64)], 1).astype(np.int64)


def border_cloud(full_scale):
    """Voxels on the borders of a field of `full_scale` voxels per axis.  -> (coords, pairs): pairs = [(i, j, (dx, dy, dz))], point
    indices of voxels that are NOT neighbours, but where the step from i overflows an axis' 12-bit key field at full_scale = 4096
    and, the fields ORed together as k_rulebook_subm does, lands on j's key: (m, y, z, 0) / (0, y, z, 1), (x, m, z, 0) /
    (x + 1, 0, z, 0), (x, y, m, 0) / (x, y + 1, 0, 0).  The kernel probes offsets 0 .. 12 only (dx <= 0) and mirrors its hits, so the
    last three pairs take their +y / +z step together with dx = -1, or dy = -1: those are steps the kernel itself makes."""
    m, a, b = full_scale - 1, full_scale // 4 + 2, full_scale // 2 + 4   # a, b even: bit 0 of the field the carry lands in is free
    pts = [(m, a, b, 0), (0, a, b, 1),          # +x of the first carries into the batch field
           (a, m, b, 0), (a + 1, 0, b, 0),      # +y carries into x
           (a, b, m, 0), (a, b + 1, 0, 0),      # +z carries into y
           (m, b, a, 2), (0, b + 1, a - 1, 3),  # a diagonal step with the x carry
           (a + 1, m, b, 0),                    # (-1, +1, 0): x - 1 = a, y carries into it -> (a + 1, 0, b, 0) = point 3
           (a + 1, b, m, 0),                    # (-1, 0, +1): z carries into y -> (a, b + 1, 0, 0) = point 5
           (a, b + 1, m, 4), (a, b + 1, 0, 4)]  # (0, -1, +1): y - 1 = b, z carries into it
    pairs = [(0, 1, (1, 0, 0)), (2, 3, (0, 1, 0)), (4, 5, (0, 0, 1)), (6, 7, (1, 1, -1)),
             (8, 3, (-1, 1, 0)), (9, 5, (-1, 0, 1)), (10, 11, (0, -1, 1))]
    # true neighbours beside voxels at 0 and at m of every axis, corners included
    for base, s in ((0, 1), (m, -1)):
        pts += [(base, base, base, 0), (base + s, base, base, 0), (base, base + s, base, 0), (base, base, base + s, 0),
                (base + s, base + s, base + s, 0)]
        for step in (2, 4):   # ... which stay neighbours of the border voxel at the coarse levels (size full_scale >> l)
            pts += [(base + s * step, base, base, 0), (base, base + s * step, base, 0), (base, base, base + s * step, 0)]
        pts += [(base, a, b, 0), (base + s, a, b + 1, 0), (a, base, b, 0), (a - 1, base + s, b, 0), (a, b, base, 0), (a + 1, b, base + s, 0)]
    # the same voxel in another batch is no neighbour of anything in batch 0
    pts += [(0, 0, 0, 1), (m, m, m, 1)]
    return np.asarray(pts, np.int64), pairs


def subm_model(row_keys, size, limit=None):
    """The loop of k_rulebook_subm in numpy: offsets 0 .. 12 probed, every hit mirrored into offset 26 - o, the query key made
    by ORing the stepped fields together.  `limit`: the last coordinate the range test lets through (size - 1 in the kernel;
    `size` = the test off by one, which lets an overflowing field carry into the next one)."""
    limit = size - 1 if limit is None else limit
    k = row_keys.astype(np.int64)
    A = len(k)
    look = scn3d._Lookup(row_keys)
    nbr = np.full((27, A), -1, np.int32)
    nbr[13] = np.arange(A)
    for o in range(13):
        x, y, z = ((k >> 24) & 4095) + o // 9 - 1, ((k >> 12) & 4095) + (o // 3) % 3 - 1, (k & 4095) + o % 3 - 1
        ok = (x >= 0) & (x <= limit) & (y >= 0) & (y <= limit) & (z >= 0) & (z <= limit)
        q = (k & ~0xFFFFFFFFF) | (x << 24) | (y << 12) | z
        r = np.where(ok, look(np.where(ok, q, k).astype(np.uint64)), -1)
        nbr[o] = r
        hit = np.nonzero(r >= 0)[0]
        nbr[26 - o, r[hit]] = hit
    return nbr


def stride2_cases():
    """name -> coords (N,4) of distinct voxels for the stride-2 tables."""
    octs = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    all8 = [(10 + x, 20 + y, 30 + z, 0) for x, y, z in octs]
    one_each = [(2 * (3 + i) + x, 2 * (5 + 2 * i) + y, 2 * (7 + i) + z, 0) for i, (x, y, z) in enumerate(octs)]
    return {"all_8_children": np.asarray(all8, np.int64),
            "one_child_per_octant": np.asarray(one_each[::-1] + [(40, 40, 40, 1)], np.int64),
            "all_8_and_single_children": np.asarray(one_each[:4] + all8 + one_each[4:], np.int64),
            "num_coarse_1": np.asarray([(7, 9, 11, 0), (6, 8, 10, 0), (7, 8, 11, 0)], np.int64)}


def distinct_keys(n, seed, box=41, batches=3):
    """n distinct voxel keys inside a box^3 x batches region, in random order (many share their parent)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lin = rng.choice(box ** 3 * batches, n, replace=False)
    c = np.stack([lin % box, (lin // box) % box, (lin // box ** 2) % box, lin // box ** 3], 1).astype(np.int64)
    return scn3d.pack_keys(c)


def coarsen_reference(fine_keys):
    """-> (coarse keys in first-seen order, parent of every fine key)."""
    c = scn3d.unpack_keys(fine_keys)
    c[:, :3] >>= 1
    ck, parent = scn3d.first_seen_unique(scn3d.pack_keys(c))
    return ck, parent.astype(np.int32)


# model of csrc/hash3d.hip::home_slot + linear probing, used only to show that the lattice DOES wrap at the end of the table
def home_slot_model(keys, cap):
    k = np.asarray(keys, np.uint64)
    blk = k & ~np.uint64(0x003003003)
    local = (((k >> np.uint64(24)) & np.uint64(3)) << np.uint64(4)) | (((k >> np.uint64(12)) & np.uint64(3)) << np.uint64(2)) | (k & np.uint64(3))
    h = blk.copy()
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xff51afd7ed558ccd)
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xc4ceb9fe1a85ec53)
    h ^= h >> np.uint64(33)
    return ((((h & np.uint64(0xFFFFFFFF)) << np.uint64(6)) | local) & np.uint64(cap - 1)).astype(np.int64), local.astype(np.int64)


def probe_model(keys, cap):
    """Insert distinct keys one after the other.  -> (longest probe chain, keys whose chain crossed a 64-slot bucket end, keys
    whose chain wrapped from slot cap - 1 to slot 0).  The set of occupied slots, and with it the number of wraps, does not depend on
    the insertion order."""
    home, _ = home_slot_model(keys, cap)
    used = np.zeros(cap, bool)
    longest = crossed = wrapped = 0
    for h in home.tolist():
        s, steps = h, 0
        while used[s]:
            s = (s + 1) & (cap - 1)
            steps += 1
        used[s] = True
        longest = max(longest, steps)
        crossed += (h + steps) // 64 != h // 64
        wrapped += h + steps >= cap
    return longest, crossed, wrapped


# ------------------------------------------------------------------------------------------------ point CSR
def csr_cases():
    """name -> (point_row int32 [N], num_rows)."""
    rng = np.random.Generator(np.random.PCG64(5))
    out = {"one_point": (np.zeros(1, np.int32), 1)}
    pr = np.concatenate([np.full(3000, 17), rng.integers(0, 40, 500)])
    out["one_row_holds_3000_of_3500"] = (pr[rng.permutation(3500)].astype(np.int32), 40)
    out["20000_points_9000_rows"] = (rng.integers(0, 9000, 20000).astype(np.int32), 9000)      # > 8192 rows: the three-launch scan
    out["5000_points_12000_rows_mostly_empty"] = (rng.integers(1, 11999, 5000).astype(np.int32), 12000)   # first and last row empty
    return out


def csr_reference(point_row, num_rows):
    """row_start [num_rows + 1], row_points [N]: the points of each row in increasing point index."""
    cnt = np.bincount(point_row.astype(np.int64), minlength=num_rows)
    row_start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    return row_start, np.argsort(point_row, kind="stable").astype(np.int32)


# ------------------------------------------------------------------------------------------------ grouped rulebook
RB_COUNTS = [0, 1, 15, 16, 17, 32, 33, 48, 49, 64]      # rules of one (tile, offset): ceil(n / 16) groups
RB_SHAPES = [(K, A) for K in (27, 8) for A in (1, 63, 64, 65, 128, 129)]


def rb_table(K, A, seed=0, rows_in=1000):
    """A synthetic rule table nbr[K][A] (int32, -1 = no rule) whose (tile, offset) pairs hold RB_COUNTS[...] rules (as many as
    the tile has rows, in a last partial tile), on random lanes, pointing at random input rows."""
    rng = np.random.Generator(np.random.PCG64(1000 * K + A + seed))
    nbr = np.full((K, A), -1, np.int32)
    for t in range((A + 63) // 64):
        rows = min(64, A - 64 * t)
        for o in range(K):
            n = min(RB_COUNTS[(t * K + o + seed) % len(RB_COUNTS)], rows)
            lanes = np.sort(rng.choice(rows, n, replace=False))
            nbr[o, 64 * t + lanes] = rng.integers(0, rows_in, n)
    return nbr


def rb_counts_hit(nbr):
    """The set of per-(tile, offset) rule counts of a table."""
    K, A = nbr.shape
    return {int((nbr[o, 64 * t:64 * t + 64] >= 0).sum()) for t in range((A + 63) // 64) for o in range(K)}


def rb_reference(nbr):
    """The layout documented above k_rb_count (csrc/spconv.hip): tile t = output rows 64 t .. 64 t + 63 owns the groups
    grp_start[t] .. grp_start[t + 1] - 1, ordered by filter offset; the n rules of one (tile, offset) fill ceil(n / 16) groups of 16
    slots in the order of their lane (row within the tile), -1 pads the last one.
    -> (tile_groups [tiles], grp_start [tiles + 1], grp_o [G], grp_in [G][16], grp_out [G][16])"""
    K, A = nbr.shape
    tiles = (A + 63) // 64
    tile_groups = np.zeros(tiles, np.int64)
    go, gi, gout = [], [], []
    for t in range(tiles):
        for o in range(K):
            row = nbr[o, 64 * t:64 * t + 64]
            lanes = np.nonzero(row >= 0)[0]
            if lanes.size == 0:
                continue
            ng = (lanes.size + 15) // 16
            pad = np.full(ng * 16 - lanes.size, -1, np.int64)
            go += [o] * ng
            gi.append(np.concatenate([row[lanes].astype(np.int64), pad]))
            gout.append(np.concatenate([lanes.astype(np.int64), pad]))
            tile_groups[t] += ng
    G = len(go)
    grp_start = np.concatenate([[0], np.cumsum(tile_groups)])
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0, np.int64)).reshape(G, 16)   # noqa: E731
    return tile_groups, grp_start, np.asarray(go, np.int64), cat(gi), cat(gout)


def rb_group_bound(K, A):
    """The number of groups Geometry3D sizes a table's share of the group arrays from (mopa_amd/sparse3d.py)."""
    return K * ((A + 15) // 16 + (A + 63) // 64)


def rb_triples(grp_start, grp_o, grp_in, grp_out):
    """A grouped rulebook back as sorted (offset, input row, output row) triples."""
    out = []
    for t in range(len(grp_start) - 1):
        for g in range(int(grp_start[t]), int(grp_start[t + 1])):
            for s in range(16):
                if grp_in[g][s] >= 0:
                    out.append((int(grp_o[g]), int(grp_in[g][s]), 64 * t + int(grp_out[g][s])))
    return sorted(out)


def table_triples(nbr):
    o, i = np.nonzero(nbr >= 0)
    return sorted(zip(o.tolist(), nbr[o, i].tolist(), i.tolist()))


# ------------------------------------------------------------------------------------------------ voxeliser
def voxel_cases():
    """name -> (points (N,3) float32, scale, full_scale, transl_u or None).  No NaN / infinity: the reference does not define them."""
    rng = np.random.Generator(np.random.PCG64(9))
    k = np.arange(-6, 7, dtype=np.float32)
    ties = np.stack([2 * k + 1, 2 * k[::-1] + 1, 2 * np.roll(k, 3) + 1], 1)            # * 0.5 = k + 0.5 exactly, k < 0 and k > 0
    span = rng.uniform(0, 1, (500, 3)).astype(np.float32) * np.asarray([70.4, 63.0, 10.0], np.float32)
    span[:3] = [[0, 0, 0], [70.4, 63.0, 10.0], [35.2, 31.6, 5.0]]                      # axis 0 is wider than the field, axis 1 spans it
    wide = (rng.uniform(-45, 45, (800, 3))).astype(np.float32)                         # 90 voxels wide in a field of 64
    one = 1.0 - 2.0 ** -53
    return {"single_point": (np.asarray([[1.25, -3.5, 7.0]], np.float32), 20.0, 4096, None),
            "single_point_translated": (np.asarray([[1.25, -3.5, 7.0]], np.float32), 20.0, 4096, (0.3, 0.6, 0.9)),
            "ties_to_even": (ties, 0.5, 4096, None),
            "ties_to_even_translated_u0": (ties, 0.5, 64, (0.0, 0.0, 0.0)),
            "span_u0": (span, 1.0, 64, (0.0, 0.0, 0.0)),
            "span_u_just_below_1": (span, 1.0, 64, (one, one, one)),
            "span_no_translation": (span, 1.0, 64, None),
            "wider_than_the_field": (wide, 1.0, 64, None),
            "wider_than_the_field_translated": (wide, 1.0, 64, (0.25, one, 0.0))}
