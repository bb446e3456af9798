"""mopa_amd/ground.py without a device: the zone model's numbering, the float64 numpy restatement of the ground estimate
(tests/_ground_reference.py, the yardstick of tests/test_gpu_ground.py) on the synthetic sweeps, the argument checks and the
``g_indices`` file layout."""
import numpy as np
import pytest
import torch

import _ground_reference as ref
from mopa_amd import ground, synth


def test_the_patch_numbering_adds_up_and_matches_a_brute_force_table():
    table = ref.patch_table()
    assert table.shape == (504, 3) == (ref.N_PATCHES, 3)
    assert sum(r * s for r, s in zip(ref.RINGS, ref.SECTORS)) == 504
    assert [int(np.nonzero(table[:, 0] == k)[0][0]) for k in range(4)] == list(ref.ZONE_PATCH0)
    from mopa_amd import _lib
    assert _lib.query("mopa_ground_patches") == 504
    # the centre of every cell of the zone model, enumerated zone-major, then ring, then sector, gets its position as id
    b = ref.zone_bounds(2.7, 80.0)
    pts = []
    for k, ring, sector in table:
        rw = (b[k + 1] - b[k]) / ref.RINGS[k]
        r = b[k] + (ring + 0.5) * rw
        th = (sector + 0.5) * 2 * np.pi / ref.SECTORS[k]
        pts.append((r * np.cos(th), r * np.sin(th), -1.0))
    pid, fragile = ref.patch_ids(np.array(pts, np.float32), 1.84)
    assert np.array_equal(pid, np.arange(504)) and not fragile.any()
    # the global ring index runs 0..13
    rings = np.concatenate([ref.ZONE_RING0[k] + np.repeat(np.arange(ref.RINGS[k]), ref.SECTORS[k]) for k in range(4)])
    assert rings.min() == 0 and rings.max() == 13 and np.array_equal(np.unique(rings), np.arange(14))
    # outside [rmin, rmax), a non-finite coordinate, a zone-0 point below -1.1 h: in no patch
    odd = np.array([[1.0, 1.0, -1.8], [80.0, 0.5, -1.8], [60.0, 60.0, -1.8], [np.nan, 1.0, 0.0], [5.0, np.inf, 0.0], [5.0, 1.0, -np.inf],
                    [5.0, 1.0, -1.1 * 1.84 - 0.01], [30.0, 1.0, -1.1 * 1.84 - 0.01], [5.0, 1.0, -1.1 * 1.84 + 0.01]], np.float32)
    pid, _ = ref.patch_ids(odd, 1.84)
    assert (pid[:7] == -1).all() and (pid[7:] >= 0).all()


@pytest.mark.parametrize("shape", ["NUSCENES", "KITTI"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_restatement_finds_the_generators_ground(shape, seed):
    """Recall and precision against the generator's own truth (|z + h| < 0.1 within range) are both at least 0.97, and at most
    0.1 % of a sweep hangs on a comparison inside the margins (measured: 32 of 34,880 and 64-68 of 120,000 -- the sweep's first
    azimuth is -pi, where y rounds to a tiny negative float32 and theta lands on the sector boundary at pi, once per beam)."""
    spec = getattr(synth, shape)
    P, h = synth.lidar_points(seed, spec), spec["height"]
    mask, fragile = ref.estimate(P, h)
    r = np.hypot(P[:, 0].astype(np.float64), P[:, 1].astype(np.float64))
    truth = (np.abs(P[:, 2] + h) < 0.1) & (r >= 2.7) & (r < 80.0)
    tp = int((mask.astype(bool) & truth).sum())
    recall, precision = tp / int(truth.sum()), tp / int(mask.sum())
    print(f"{shape} seed {seed}: {len(P)} points, ground {int(mask.sum())}, recall {recall:.4f}, precision {precision:.4f}, fragile {int(fragile.sum())}")
    assert recall >= 0.97 and precision >= 0.97
    assert fragile.sum() <= 0.001 * len(P)


def test_a_tilted_sweep_still_has_ground():
    P = synth.lidar_points(0).astype(np.float64)
    a = np.deg2rad(4.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    mask, fragile = ref.estimate((P @ R.T).astype(np.float32), synth.NUSCENES["height"])
    assert mask.sum() > 10000 and fragile.sum() <= 0.001 * len(P)


# ------------------------------------------------------------------------------------------------ the binding, no device needed
def test_params_are_checked():
    p = ground.GroundParams(sensor_height=1.84)
    a = p.as_array()
    assert a.dtype == np.float64 and a[0] == 1.84 and a[1] == 2.7 and a[2] == 80.0 and list(a[15:18]) == [10, 20, 3]
    from mopa_amd import _lib
    assert a.size == _lib.query("mopa_ground_num_params")
    assert {k: getattr(p, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    with pytest.raises(TypeError):
        ground.GroundParams()                                   # sensor_height is required
    for bad in (dict(sensor_height=float("nan")), dict(sensor_height="1.8"), dict(sensor_height=1.8, rmin=0.0),
                dict(sensor_height=1.8, rmin=90.0), dict(sensor_height=1.8, num_min_pts=2), dict(sensor_height=1.8, num_lpr=0),
                dict(sensor_height=1.8, num_iter=2.5), dict(sensor_height=1.8, elevation=(1, 2, 3)),
                dict(sensor_height=1.8, flatness=(1, 2, 3, float("inf")))):
        with pytest.raises(ValueError):
            ground.GroundParams(**bad)


def test_arguments_are_checked_before_any_device_is_touched():
    p = ground.GroundParams(sensor_height=1.84)
    ok = np.zeros((5, 3), np.float32)
    with pytest.raises(TypeError, match="GroundParams"):
        ground.estimate_ground(ok, dict(sensor_height=1.84))
    with pytest.raises(TypeError, match="half precision"):
        ground.estimate_ground(ok.astype(np.float16), p)
    with pytest.raises(TypeError, match="half precision"):
        ground.estimate_ground(torch.zeros(5, 3, dtype=torch.bfloat16), p)
    with pytest.raises(TypeError, match="float32"):
        ground.estimate_ground(ok.astype(np.float64), p)
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        ground.estimate_ground([[0.0, 0.0, 0.0]], p)
    with pytest.raises(ValueError, match=r"\(N, >=3\)"):
        ground.estimate_ground(np.zeros((5, 2), np.float32), p)
    with pytest.raises(ValueError, match=r"\(N, >=3\)"):
        ground.estimate_ground(np.zeros(15, np.float32), p)
    with pytest.raises(ValueError, match="no scans"):
        ground.estimate_ground_batch([], p)
    with pytest.raises(TypeError, match="list"):
        ground.estimate_ground_batch(ok, p)
    with pytest.raises(ValueError, match="one width per call"):
        ground.estimate_ground_batch([ok, np.zeros((5, 4), np.float32)], p)
    with pytest.raises(ValueError, match="add up"):
        ground.estimate_ground_batch(ok, p, counts=[2, 2])
    with pytest.raises(ValueError, match="negative"):
        ground.estimate_ground_batch(ok, p, counts=[6, -1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ground.estimate_ground(ok, p, device="cpu")


def test_dump_g_indices_round_trips_through_fromfile(tmp_path):
    rng = np.random.Generator(np.random.PCG64(5))
    mask = (rng.random(1000) < 0.4).astype(np.uint8)
    idx = ground.ground_indices(torch.from_numpy(mask))
    assert idx.dtype == torch.int32 and np.array_equal(idx.numpy(), np.nonzero(mask)[0])
    assert np.array_equal(ground.ground_indices(mask.astype(bool)).numpy(), np.nonzero(mask)[0])
    path = tmp_path / "scan.bin"
    assert ground.dump_g_indices(path, torch.from_numpy(mask)) == int(mask.sum())
    back = np.fromfile(path, dtype=np.int32)                    # what the reference's datasets do with the file
    g_mask = np.zeros(1000)
    g_mask[back] = 1
    assert np.array_equal(g_mask.astype(bool), mask.astype(bool))
    assert ground.dump_g_indices(tmp_path / "none.bin", np.zeros(7, np.uint8)) == 0
    assert np.fromfile(tmp_path / "none.bin", dtype=np.int32).size == 0
    with pytest.raises(TypeError):
        ground.ground_indices(np.zeros((3, 3), np.uint8))
    with pytest.raises(TypeError):
        ground.ground_indices(np.zeros(3, np.float32))
