"""mopa_amd/ground.py on the device (csrc/ground.hip) against the float64 numpy restatement tests/_ground_reference.py.

The condition of every comparison: the device mask equals the restatement's mask on every point that the restatement does not
flag as fragile (a comparison within 1e-9 relative of a bin boundary or 1e-6 of a threshold, see the restatement's docstring), and
the fragile points are at most 0.1 % of the case.  The small cases are built with every quantity far from its threshold: they have
no fragile point at all, which ``compare`` asserts for them.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch

import _ground_reference as ref
from mopa_amd import synth

pytestmark = pytest.mark.gpu

H = 1.84
F32 = np.float32
BOUNDS = ref.zone_bounds(2.7, 80.0)


def params(h=H, **kw):
    from mopa_amd import ground
    return ground.GroundParams(sensor_height=h, **kw)


def cell(rng, n, zone, ring, sector, z, margin=0.1):
    """n points spread over the inner part of one cell of the zone model (a `margin` share of its width stays free on every
    side), at height z (a number, or a function of (r, theta) -> (n,))."""
    rw = (BOUNDS[zone + 1] - BOUNDS[zone]) / ref.RINGS[zone]
    sa = 2 * np.pi / ref.SECTORS[zone]
    r = BOUNDS[zone] + (ring + rng.uniform(margin, 1 - margin, n)) * rw
    th = (sector + rng.uniform(margin, 1 - margin, n)) * sa
    zz = z(r, th) if callable(z) else np.full(n, float(z))
    return np.stack([r * np.cos(th), r * np.sin(th), zz], 1).astype(F32)


def flat(rng, sigma=0.02, at=-H):
    return lambda r, th: at + rng.normal(0.0, sigma, r.shape)


def patch_of(zone, ring, sector):
    return ref.ZONE_PATCH0[zone] + ring * ref.SECTORS[zone] + sector


def tilted(P, deg=4.0):
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return (P.astype(np.float64) @ R.T).astype(F32)


def build_cases():
    """name -> (points, sensor height, whether the case must have no fragile point)."""
    from mopa_amd import _lib
    cap = _lib.query("mopa_ground_resident_capacity")
    rng = np.random.Generator(np.random.PCG64(2024))
    c = {}
    c["no points"] = np.zeros((0, 3), F32)
    c["one point"] = np.array([[10.0, 3.0, -H]], F32)
    th = rng.uniform(0, 2 * np.pi, 500)
    rr = rng.uniform(0.0, 2.6, 500)
    c["all inside rmin"] = np.stack([rr * np.cos(th), rr * np.sin(th), rng.normal(-H, 0.02, 500)], 1).astype(F32)
    # a ring of flat cells; rows with NaN / inf in any column (also in otherwise valid ground points) are in no patch
    base = np.concatenate([cell(rng, 60, 2, 1, s, flat(rng)) for s in range(0, 54, 3)])
    bad = base.copy()
    rows = rng.choice(len(bad), 90, replace=False)
    bad[rows[:30], 0] = np.nan
    bad[rows[30:50], 1] = np.inf
    bad[rows[50:70], 2] = -np.inf
    bad[rows[70:], 2] = np.nan
    c["nan and inf rows"] = bad
    # both sides of num_min_pts = 10 and num_lpr = 20
    c["patches of 9 10 19 20 21"] = np.concatenate([cell(rng, n, 2, 2, 5 + 4 * j, flat(rng)) for j, n in enumerate((9, 10, 19, 20, 21))])
    # 12 points -> the LPR is their mean; 2 (3) low points well below it are the whole seed set: no fit (a three-point plane)
    def low_and_high(n_low, sector):
        low = cell(rng, n_low, 2, 1, sector, flat(rng, 0.005, -3.0), margin=0.2)
        high = cell(rng, 12 - n_low, 2, 1, sector, flat(rng, 0.005, 0.0), margin=0.2)
        return np.concatenate([high[:5], low, high[5:]])
    tri = low_and_high(3, 20)
    lowrows = np.nonzero(tri[:, 2] < -2)[0]
    r0, t0 = BOUNDS[2] + 1.5 * (BOUNDS[3] - BOUNDS[2]) / 4, 20.5 * 2 * np.pi / 54     # a well-shaped triangle around the cell's centre:
    #                                                                                   the three seeds must not be collinear
    tri[lowrows, 0] = [F32((r0 + dr) * np.cos(t0 + dt)) for dr, dt in ((-1.0, -0.02), (1.0, -0.02), (0.0, 0.03))]
    tri[lowrows, 1] = [F32((r0 + dr) * np.sin(t0 + dt)) for dr, dt in ((-1.0, -0.02), (1.0, -0.02), (0.0, 0.03))]
    c["seed sets of 2 and 3"] = np.concatenate([low_and_high(2, 10), tri])
    # one sector just below and one just above what the fit kernel keeps in LDS: a plane, noise, and a tenth of clutter above it
    def full_sector(n, sector):
        def z(r, th):
            zz = -H + 0.01 * (r - 8.0) + rng.normal(0.0, 0.02, r.shape)
            up = rng.random(r.shape) < 0.1
            return np.where(up, zz + rng.uniform(0.3, 2.0, r.shape), zz)
        return cell(rng, n, 1, 1, sector, z, margin=0.02)
    c["below and above the resident capacity"] = np.concatenate([full_sector(cap - 3, 4), full_sector(cap, 9), full_sector(cap + 1, 14),
                                                                 full_sector(cap + 700, 19)])
    # a vertical wall (an arc of constant range): the fitted normal is radial
    def wall(n, zone, ring, sector):
        rw = (BOUNDS[zone + 1] - BOUNDS[zone]) / ref.RINGS[zone]
        sa = 2 * np.pi / ref.SECTORS[zone]
        r = BOUNDS[zone] + (ring + 0.5) * rw + rng.normal(0.0, 0.01, n)
        t = (sector + rng.uniform(0.1, 0.9, n)) * sa
        return np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-1.5, 1.0, n)], 1).astype(F32)
    c["vertical wall"] = np.concatenate([wall(300, 2, 1, 7), cell(rng, 200, 2, 1, 30, flat(rng))])
    # ring 1 (zone 0, second ring), 1 m above the road: a flat slab passes the flatness test, a rough blob does not
    c["elevated slab and blob"] = np.concatenate([cell(rng, 400, 0, 1, 3, flat(rng, 0.004, -H + 1.0)),
                                                  cell(rng, 400, 0, 1, 9, lambda r, t: -H + 1.5 + rng.uniform(-0.5, 0.5, r.shape)),
                                                  cell(rng, 400, 0, 1, 13, flat(rng))])
    # zone-0 returns below -1.1 h (reflections) would drag the LPR down; they are in no patch and never ground
    c["zone 0 below the cut"] = np.concatenate([cell(rng, 300, 0, 0, 2, flat(rng)), cell(rng, 40, 0, 0, 2, flat(rng, 0.05, -1.1 * H - 0.6)),
                                                cell(rng, 300, 1, 0, 2, flat(rng)), cell(rng, 40, 1, 0, 2, flat(rng, 0.05, -1.1 * H - 0.6))])
    out = {k: (v, H, True) for k, v in c.items()}
    out["nuScenes sweep"] = (synth.lidar_points(0, synth.NUSCENES), synth.NUSCENES["height"], False)
    out["SemanticKITTI sweep"] = (synth.lidar_points(1, synth.KITTI), synth.KITTI["height"], False)
    out["tilted sweep"] = (tilted(synth.lidar_points(0, synth.NUSCENES)), synth.NUSCENES["height"], False)
    return out


NAMES = ["no points", "one point", "all inside rmin", "nan and inf rows", "patches of 9 10 19 20 21", "seed sets of 2 and 3",
         "below and above the resident capacity", "vertical wall", "elevated slab and blob", "zone 0 below the cut", "nuScenes sweep",
         "SemanticKITTI sweep", "tilted sweep"]


@pytest.fixture(scope="module")
def cases():
    """Every case with the restatement's answer, computed once: name -> dict(P, h, clean, mask, fragile)."""
    built = build_cases()
    assert sorted(built) == sorted(NAMES)
    out = {}
    for name, (P, h, clean) in built.items():
        mask, fragile = ref.estimate(P, h)
        out[name] = dict(P=P, h=h, clean=clean, mask=mask, fragile=fragile)
    return out


def compare(name, c, got):
    """The condition of the module docstring."""
    got = got.cpu().numpy()
    n = len(c["P"])
    assert got.dtype == np.uint8 and got.shape == (n,) and set(np.unique(got)) <= {0, 1}
    nf = int(c["fragile"].sum())
    wrong = int(((got != c["mask"]) & ~c["fragile"]).sum())
    print(f"{name}: {n} points, ground {int(c['mask'].sum())} (device {int(got.sum())}), fragile {nf}, differing outside them {wrong}")
    assert nf <= 0.001 * n and (nf == 0 or not c["clean"]), f"{name}: {nf} fragile points of {n}"
    assert wrong == 0, f"{name}: {wrong} non-fragile points differ"


def pids(c):
    return ref.patch_ids(c["P"], c["h"])[0]


# ------------------------------------------------------------------------------------------------ the restatement on the cases
def test_the_cases_test_what_they_are_named_for(cases):
    """The restatement alone, so that a case cannot pass by being empty: each one exercises the branch it is there for."""
    from mopa_amd import _lib
    cap = _lib.query("mopa_ground_resident_capacity")
    c = cases["all inside rmin"]
    assert (pids(c) == -1).all() and c["mask"].sum() == 0
    c = cases["nan and inf rows"]
    bad = ~np.isfinite(c["P"]).all(1)
    assert bad.sum() == 90 and (pids(c)[bad] == -1).all() and c["mask"][bad].sum() == 0 and c["mask"].sum() > 500
    c = cases["patches of 9 10 19 20 21"]
    sizes = {n: patch_of(2, 2, 5 + 4 * j) for j, n in enumerate((9, 10, 19, 20, 21))}
    for n, p in sizes.items():
        sel = pids(c) == p
        assert sel.sum() == n and (c["mask"][sel].sum() > 0) == (n >= 10)
    c = cases["seed sets of 2 and 3"]
    two, three = pids(c) == patch_of(2, 1, 10), pids(c) == patch_of(2, 1, 20)
    assert two.sum() == 12 and three.sum() == 12 and c["mask"][two].sum() == 0 and c["mask"][three].sum() == 3
    assert (c["P"][three & (c["mask"] == 1), 2] < -2).all()
    c = cases["below and above the resident capacity"]
    for n, s in ((cap - 3, 4), (cap, 9), (cap + 1, 14), (cap + 700, 19)):
        sel = pids(c) == patch_of(1, 1, s)
        assert sel.sum() == n and 0.8 * n < c["mask"][sel].sum() < 0.95 * n
    c = cases["vertical wall"]
    wall = pids(c) == patch_of(2, 1, 7)
    assert wall.sum() == 300 and c["mask"][wall].sum() == 0 and c["mask"][~wall].sum() > 150
    c = cases["elevated slab and blob"]
    slab, blob, road = (pids(c) == patch_of(0, 1, s) for s in (3, 9, 13))
    assert c["mask"][slab].sum() > 350 and c["mask"][blob].sum() == 0 and c["mask"][road].sum() > 350
    c = cases["zone 0 below the cut"]
    low = c["P"][:, 2] < -1.1 * H
    z0 = np.hypot(c["P"][:, 0], c["P"][:, 1]) < BOUNDS[1]
    assert (pids(c)[low & z0] == -1).all() and (pids(c)[low & ~z0] >= 0).all() and c["mask"][low & z0].sum() == 0
    assert c["mask"][z0 & ~low].sum() > 250                 # zone 0 keeps its road: the reflections are not its lowest points
    for name in ("nuScenes sweep", "SemanticKITTI sweep", "tilted sweep"):
        assert cases[name]["mask"].sum() > 10000
    assert np.bincount(pids(cases["SemanticKITTI sweep"])[pids(cases["SemanticKITTI sweep"]) >= 0]).max() > cap   # the streaming form


# ------------------------------------------------------------------------------------------------ the device against it
@pytest.mark.parametrize("name", NAMES)
def test_the_device_mask_equals_the_restatement(cases, name):
    from mopa_amd import ground
    c = cases[name]
    got = ground.estimate_ground(c["P"], params(c["h"]))
    assert got.is_cuda and got.dtype == torch.uint8
    compare(name, c, got)


@pytest.mark.parametrize("names", [("vertical wall",), ("nuScenes sweep", "elevated slab and blob"),
                                   ("SemanticKITTI sweep", "seed sets of 2 and 3", "no points", "below and above the resident capacity",
                                    "one point")])
def test_a_batch_equals_the_scans_one_by_one(cases, names):
    """1, 2 and 5 scans of unequal sizes, an empty one in the middle: one call for the list, the masks of the per-scan calls.  (One
    sensor height per call: the SemanticKITTI sweep is judged against the restatement at the height the call uses.)"""
    from mopa_amd import ground
    h = cases[names[0]]["h"]
    sets = [cases[n]["P"] for n in names]
    got = ground.estimate_ground_batch(sets, params(h))
    assert len(got) == len(sets) and [g.shape[0] for g in got] == [len(p) for p in sets]
    for n, p, g in zip(names, sets, got):
        assert torch.equal(g, ground.estimate_ground(p, params(h))), n
        if cases[n]["h"] == h:
            compare(n, cases[n], g)
    # the same list as one concatenated array with counts (what kittiprep hands on), with a fourth column that is not read
    cat = np.concatenate(sets, 0)
    cat4 = torch.from_numpy(np.concatenate([cat, np.full((len(cat), 1), np.nan, F32)], 1)).cuda()
    again = ground.estimate_ground_batch(cat4, params(h), counts=[len(p) for p in sets])
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_two_runs_leave_the_same_bits(cases):
    from mopa_amd import ground
    sets = [cases[n]["P"] for n in ("SemanticKITTI sweep", "nuScenes sweep", "below and above the resident capacity")]
    dev = [torch.from_numpy(p).cuda() for p in sets]
    a = ground.estimate_ground_batch(dev, params(1.73))
    b = ground.estimate_ground_batch(dev, params(1.73))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and sum(int(x.sum()) for x in a) > 50000


def test_host_and_device_inputs_give_the_same_mask(cases):
    from mopa_amd import ground
    P = cases["nuScenes sweep"]["P"]
    want = ground.estimate_ground(P, params())
    assert torch.equal(want, ground.estimate_ground(torch.from_numpy(P), params()))             # a host tensor
    assert torch.equal(want, ground.estimate_ground(torch.from_numpy(P).cuda(), params()))      # a device tensor
    wide = torch.from_numpy(np.concatenate([P, np.ones((len(P), 2), F32)], 1)).cuda()
    assert torch.equal(want, ground.estimate_ground(wide, params()))                            # (N, 5): only x, y, z are read
    mixed = ground.estimate_ground_batch([P, torch.from_numpy(P).cuda()], params())
    assert torch.equal(mixed[0], want) and torch.equal(mixed[1], want)


def test_ground_indices_are_nonzero(cases, tmp_path):
    from mopa_amd import ground
    c = cases["nuScenes sweep"]
    mask = ground.estimate_ground(c["P"], params())
    idx = ground.ground_indices(mask)
    assert idx.is_cuda and idx.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), np.nonzero(mask.cpu().numpy())[0])
    assert ground.dump_g_indices(tmp_path / "g.bin", mask) == int(mask.sum())
    assert np.array_equal(np.fromfile(tmp_path / "g.bin", dtype=np.int32), idx.cpu().numpy())


def test_other_parameters_reach_the_kernels(cases):
    """The record is read, not the defaults: other thresholds, the same agreement."""
    from mopa_amd import ground
    c = cases["nuScenes sweep"]
    kw = dict(num_min_pts=25, num_lpr=7, num_iter=2, th_seeds=0.2, th_dist=0.08, uprightness=0.9, rmin=4.0, rmax=60.0)
    mask, fragile = ref.estimate(c["P"], c["h"], **kw)
    assert (mask != c["mask"]).sum() > 100
    compare("other parameters", dict(c, mask=mask, fragile=fragile), ground.estimate_ground(c["P"], params(c["h"], **kw)))


# ------------------------------------------------------------------------------------------------ the chain into VGI
def test_the_estimate_feeds_point_mixmatch():
    """point_mixmatch(..., g_indices=estimate_ground(pc)) places the object on the road: its lowest z is the road height under the
    chosen cell (-h up to the sweep's 0.02 m noise; three sigma are allowed) plus the reference's jitter in [0, 0.1).  Without a
    mask the call still raises."""
    from mopa_amd import ground, vgi
    from oracle.gen_golden import vgi_case
    c = vgi_case(0)
    kw = dict(insert_mode="ground", search_voxel_size=0.5, search_range=[25.0, 25.0], search_z_min=-2.0, proj_matrix=c["proj"],
              image_size=c["image_size"], front_axis=c["front"])
    pc = torch.from_numpy(c["ori_pc"]).cuda()
    g = ground.estimate_ground(pc, params(synth.NUSCENES["height"]))
    assert g.shape == (len(c["ori_pc"]),) and int(g.sum()) > 10000
    np.random.seed(100)
    cat_pc, cat_label, mask, _ = vgi.point_mixmatch(pc, c["label"], [o.copy() for o in c["objs"]], c["obj_labels"], g_indices=g, **kw)
    n0 = len(c["ori_pc"])
    assert int(mask.sum()) == sum(len(o) for o in c["objs"]) and not bool(mask[:n0].any())
    at = n0
    for o in c["objs"]:
        lowest = float(cat_pc[at:at + len(o), 2].min())
        at += len(o)
        assert -H - 0.06 <= lowest <= -H + 0.1 + 0.06, lowest
    with pytest.raises(RuntimeError, match="a ground mask is needed"):
        vgi.point_mixmatch(pc, c["label"], [o.copy() for o in c["objs"]], c["obj_labels"], g_indices=None, **kw)
