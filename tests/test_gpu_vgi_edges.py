"""The VGI kernels (csrc/vgi.hip), entry point by entry point, at small grids and at their edges.  Run with -m gpu on an MI355X.

Every test calls the C ABI directly (mopa_amd._lib: call / query / ptr / stream) and compares with the numpy restatements of
tests/_vgi_cases.py or with oracle/vgi.py: equalities only (the inputs are chosen so that no sum depends on its order and no
pixel on a libm's last bit; tests/test_vgi_cases_host.py checks that, and that every case holds the edge it is named after).
Output buffers are larger than the contract needs and pre-filled with a sentinel that must survive behind it; workspaces are
exactly as large as the *_workspace_bytes query says, with a guard behind them; a refused call leaves every output untouched.
Two tests at the end go through mopa_amd.vgi: OverlapMap.free_cells' None, and check_overlap at voxel sizes 0.2 and 0.3.
"""
import numpy as np
import pytest
import torch

import _vgi_cases as vc
from oracle import vgi as ovgi

pytestmark = pytest.mark.gpu

INT_MAX = vc.INT_MAX
SENT = {torch.int32: -1515870811, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0xA5, torch.float64: -1.5e300}
PAD = 64


def _L():
    from mopa_amd import _lib
    return _lib


def _buf(n, dtype=torch.int32, pad=PAD):
    """n + pad elements on the device, all of them the sentinel."""
    return torch.full((n + pad,), SENT[dtype], dtype=dtype, device="cuda")


def _untouched(t, n=0):
    """The elements of a _buf behind the first n still hold the sentinel."""
    return bool((t[n:] == SENT[t.dtype]).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Ws:
    """A workspace of exactly the queried size; `ok()` = nothing was written behind it, `clean()` = nothing at all."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.t = torch.full((self.nbytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")

    def ok(self):
        return bool((self.t[self.nbytes:] == 0xA5).all())

    def clean(self):
        return bool((self.t == 0xA5).all())


def _refused(name, *args):
    with pytest.raises(RuntimeError):
        _L().call(name, *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ mopa_vgi_first_points
def _first_points(pts, n, vs, g, g_mask=None, X=None, Y=None, stride=None):
    L = _L()
    X, Y = g["X"] if X is None else X, g["Y"] if Y is None else Y
    cells = g["X"] * g["Y"] * vc.ZR
    p, first, status = _dev(pts), _buf(cells), _buf(1)
    m = None if g_mask is None else _dev(g_mask)
    L.call("mopa_vgi_first_points", L.ptr(p), pts.shape[1] if stride is None else stride, n, float(np.float32(vs)), g["ox"], g["oy"], X, Y,
           g["zlo"], L.ptr(m), L.ptr(first), L.ptr(status), L.stream())
    return first, status, cells


@pytest.mark.parametrize("n", vc.FIRST_SIZES)
@pytest.mark.parametrize("name", list(vc.MAPS))
def test_first_points_equals_the_reference(name, n):
    """n below, at and above a wave and 3000; strides 3, 4, 5; voxel sizes 0.5, 0.25, 1.0, both front axes: points on voxel faces
    (negative ones too), on the first and last cell and just outside, z slots -1, 0, 127, 128, duplicates (the smaller index
    wins); the status word with and without flags on the dropped points."""
    vs, sr, front = vc.MAPS[name]
    g = vc.map_geometry(vs, sr, front)
    pts, _ = vc.first_cloud(vs, sr, front, n)
    ref, _ = vc.ref_first_points(pts, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"])
    for stride in (3, 4, 5):
        first, status, cells = _first_points(vc.pad_stride(pts, stride), n, vs, g)
        assert np.array_equal(first[:cells].cpu().numpy(), ref), stride
        assert int(status[0]) == 0 and _untouched(first, cells) and _untouched(status, 1)
    masks, dropped = vc.first_masks(pts, vs, g)
    for kind, want in (("ground_dropped", int(dropped.any())), ("nonground_dropped", 0)):
        first, status, cells = _first_points(pts, n, vs, g, masks[kind])
        assert int(status[0]) == want == vc.ref_first_points(pts, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], masks[kind])[1], kind
        assert np.array_equal(first[:cells].cpu().numpy(), ref) and _untouched(first, cells) and _untouched(status, 1)


def test_first_points_refuses_bad_arguments():
    vs, sr, front = vc.MAPS["vs0.5_x"]
    g = vc.map_geometry(vs, sr, front)
    pts, _ = vc.first_cloud(vs, sr, front, 100)
    L = _L()
    p, first, status = _dev(pts), _buf(g["X"] * g["Y"] * vc.ZR), _buf(1)
    good = dict(stride=3, n=100, vs=0.5, X=g["X"], Y=g["Y"])
    for bad in (dict(n=0), dict(n=-5), dict(stride=2), dict(stride=0), dict(X=0), dict(Y=-1), dict(vs=0.0), dict(vs=-0.5), dict(vs=float("nan"))):
        a = dict(good, **bad)
        _refused("mopa_vgi_first_points", L.ptr(p), a["stride"], a["n"], a["vs"], g["ox"], g["oy"], a["X"], a["Y"], g["zlo"], None, L.ptr(first),
                 L.ptr(status), L.stream())
        assert _untouched(first) and _untouched(status), bad


def _first_points_rep(pts, n, vs, g, ws_short=0, vs64=None):
    L = _L()
    cells = g["X"] * g["Y"] * vc.ZR
    p, first, status = _dev(pts), _buf(cells), _buf(1)
    ws = _Ws(L.query("mopa_vgi_first_points_rep_workspace_bytes", g["X"], g["Y"]))
    L.call("mopa_vgi_first_points_rep", L.ptr(p), pts.shape[1], n, float(np.float32(vs)), float(vs if vs64 is None else vs64), g["ox"], g["oy"],
           g["X"], g["Y"], g["zlo"], L.ptr(first), L.ptr(status), L.ptr(ws.t), ws.nbytes - ws_short, L.stream())
    return first, status, cells, ws


@pytest.mark.parametrize("n", [1, 2, 65, 1500])
@pytest.mark.parametrize("vs", vc.OVERLAP_VOXEL_SIZES)
def test_first_points_rep_marks_representatives_at_their_float32_floor(vs, n):
    """The second path of the overlap test (voxel sizes that are no power of two): the first point of every float64 voxel, marked
    at its float32 floor.  At 0.5 and 0.25 that is the same map as mopa_vgi_first_points'."""
    g = vc.map_geometry(vs, vc.OVERLAP_RANGE, "x")
    scan = vc.overlap_cloud(vs)[0][:n]
    ref = vc.ref_first_points_rep(scan, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"])
    for stride in (3, 5):
        first, status, cells, ws = _first_points_rep(vc.pad_stride(scan, stride), n, vs, g)
        assert np.array_equal(first[:cells].cpu().numpy(), ref), stride
        assert int(status[0]) == 0 and _untouched(first, cells) and _untouched(status, 1) and ws.ok()
    if vs in (0.5, 0.25):
        assert np.array_equal(ref, vc.ref_first_points(scan, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"])[0])
    if n == 65:
        L = _L()
        p, first, status = _dev(scan), _buf(g["X"] * g["Y"] * vc.ZR), _buf(1)
        ws = _Ws(L.query("mopa_vgi_first_points_rep_workspace_bytes", g["X"], g["Y"]))
        good = dict(stride=3, n=n, vs=vs, vs64=vs, X=g["X"], Y=g["Y"], short=0)
        for bad in (dict(short=1), dict(n=0), dict(stride=2), dict(X=0), dict(Y=0), dict(vs=0.0), dict(vs64=0.0), dict(vs64=float("nan")),
                    dict(vs=float("nan"))):
            a = dict(good, **bad)
            _refused("mopa_vgi_first_points_rep", L.ptr(p), a["stride"], a["n"], a["vs"], a["vs64"], g["ox"], g["oy"], a["X"], a["Y"], g["zlo"],
                     L.ptr(first), L.ptr(status), L.ptr(ws.t), ws.nbytes - a["short"], L.stream())
            assert _untouched(first) and _untouched(status) and ws.clean(), bad


# ------------------------------------------------------------------------------------------------ mopa_vgi_box_free
@pytest.mark.parametrize("name", list(vc.box_cases()))
def test_box_free_equals_the_window_sum(name):
    """1x1x1, the box as large as the grid in one, two and three axes (one output cell), bz == Z, an empty grid, a full column, the
    eight corners of the slab (with full slots right outside it), the slab at slot 0 and ending at slot 128."""
    L = _L()
    c = vc.box_cases()[name]
    X, Y, Z, (bx, by, bz) = c["X"], c["Y"], c["Z"], c["box"]
    ref = vc.ref_box_free(c["first"], X, Y, c["zlo"], c["gz0"], Z, bx, by, bz)
    first, free = _dev(c["first"]), _buf(ref.size, torch.uint8)
    ws = _Ws(L.query("mopa_vgi_box_free_workspace_bytes", X, Y, Z))
    L.call("mopa_vgi_box_free", L.ptr(first), X, Y, c["zlo"], c["gz0"], Z, bx, by, bz, L.ptr(free), L.ptr(ws.t), ws.nbytes, L.stream())
    assert np.array_equal(free[:ref.size].cpu().numpy().reshape(ref.shape), ref)
    assert _untouched(free, ref.size) and ws.ok()
    free2, ws2 = _buf(ref.size, torch.uint8), _Ws(ws.nbytes)
    _refused("mopa_vgi_box_free", L.ptr(first), X, Y, c["zlo"], c["gz0"], Z, bx, by, bz, L.ptr(free2), L.ptr(ws2.t), ws2.nbytes - 1, L.stream())
    assert _untouched(free2) and ws2.clean()


@pytest.mark.parametrize("name", list(vc.BOX_REFUSED))
def test_box_free_refuses(name):
    """A box larger than the grid in any axis, a slab that leaves the 128 slots at either end, non-positive sizes."""
    L = _L()
    X, Y, gz0, Z, bx, by, bz = vc.BOX_REFUSED[name]
    first = _dev(vc.box_cases()["sparse"]["first"])
    free, ws = _buf(16 * 10 * 8, torch.uint8), _Ws(L.query("mopa_vgi_box_free_workspace_bytes", 16, 10, 8))
    _refused("mopa_vgi_box_free", L.ptr(first), X, Y, vc.ZLO, gz0, Z, bx, by, bz, L.ptr(free), L.ptr(ws.t), ws.nbytes, L.stream())
    assert _untouched(free) and ws.clean()


# ------------------------------------------------------------------------------------------------ mopa_vgi_ground_cells
@pytest.mark.parametrize("n", [1, 14, 1025, 3000])
def test_ground_cells_follow_the_first_point_rule(n):
    """A column whose only ground voxel is z slot 127, a column with both kinds of voxels, a voxel whose first point is not ground
    and whose second is (not a ground column), the other way round (a ground column)."""
    L = _L()
    pts, flags, g = vc.ground_cloud(n)
    first, _ = vc.ref_first_points(pts, g["vs"], g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], flags)
    ref = vc.ref_ground_cells(first, flags, g["X"], g["Y"])
    f, m, g2d = _dev(first), _dev(flags), _buf(g["X"] * g["Y"], torch.uint8)
    L.call("mopa_vgi_ground_cells", L.ptr(f), L.ptr(m), g["X"], g["Y"], L.ptr(g2d), L.stream())
    assert np.array_equal(g2d[:ref.size].cpu().numpy(), ref) and _untouched(g2d, ref.size)
    if n >= 14:
        at = {k: (c[0] - g["ox"]) * g["Y"] + c[1] - g["oy"] for k, c in vc.GROUND_CELLS.items()}
        assert [int(g2d[at[k]]) for k in ("top", "mixed", "late", "early", "two")] == [1, 1, 0, 1, 1]
    g2 = _buf(g["X"] * g["Y"], torch.uint8)
    for X, Y in ((0, g["Y"]), (g["X"], 0), (-1, -1)):
        _refused("mopa_vgi_ground_cells", L.ptr(f), L.ptr(m), X, Y, L.ptr(g2), L.stream())
        assert _untouched(g2)


# ------------------------------------------------------------------------------------------------ mopa_vgi_candidates
def _params(c):
    return np.concatenate([c["ext"], c["off"], [c["vs"], c["ori_range"]], c["P"].astype(np.float32).reshape(-1),
                           [float(c["image_size"][0]), float(c["image_size"][1])]]).astype(np.float64)


@pytest.mark.parametrize("name", list(vc.cand_cases()))
def test_candidates_equal_filter_centers_plus_ground_centers(name):
    """Every filter at its boundary, both front axes: cx == 0, u == 0 / img_w and v == 0 / img_h (out; one cell inside is in),
    p2 < 0, range == ori_range on a 3-4-5 centre (in), cells that are not ground, no free cell, every cell passing."""
    L = _L()
    c = vc.cand_cases()[name]
    g = c["g"]
    first, _ = vc.ref_first_points(c["scan"], c["vs"], g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], c["g_mask"])
    g2d = vc.ref_ground_cells(first, c["g_mask"], g["X"], g["Y"])
    want_cand, want_counts = vc.oracle_candidates(c)
    assert vc.ref_candidates(c["free"], c["ext"], c["off"], c["vs"], c["ori_range"], c["P"], c["image_size"], g2d, g["ox"], g["oy"], g["X"],
                             g["Y"])[1] == want_counts
    free, gd, params = _dev(c["free"]), _dev(g2d), _params(c)
    cand, counts = _buf(g["X"] * g["Y"], torch.uint8), _buf(2)
    Xo, Yo, Zo = c["free"].shape
    L.call("mopa_vgi_candidates", L.ptr(free), Xo, Yo, Zo, params.ctypes.data, L.ptr(gd), g["ox"], g["oy"], g["X"], g["Y"], L.ptr(cand),
           L.ptr(counts), L.stream())
    assert tuple(counts[:2].tolist()) == want_counts
    assert np.array_equal(cand[:g["X"] * g["Y"]].cpu().numpy(), want_cand)
    assert _untouched(cand, g["X"] * g["Y"]) and _untouched(counts, 2)
    if name == "random_free_x":
        cand2, counts2 = _buf(g["X"] * g["Y"], torch.uint8), _buf(2)
        good = dict(Xo=Xo, Yo=Yo, Zo=Zo, X=g["X"], Y=g["Y"], params=params.ctypes.data)
        for bad in (dict(Xo=0), dict(Yo=-1), dict(Zo=0), dict(X=0), dict(Y=0), dict(params=None)):
            a = dict(good, **bad)
            _refused("mopa_vgi_candidates", L.ptr(free), a["Xo"], a["Yo"], a["Zo"], a["params"], L.ptr(gd), g["ox"], g["oy"], a["X"], a["Y"],
                     L.ptr(cand2), L.ptr(counts2), L.stream())
            assert _untouched(cand2) and _untouched(counts2), bad


# ------------------------------------------------------------------------------------------------ mopa_vgi_compact_cells
@pytest.mark.parametrize("X,Y", vc.COMPACT_MAPS)
def test_compact_cells_row_major_order_and_count(X, Y):
    """Maps of 1, 1023, 1024, 1025 and 2049 cells (one, one, one, two and three trips of the 1024-thread block); nothing marked,
    everything, only the last cell, every 65th (one per wave, drifting through the lanes)."""
    L = _L()
    ox, oy = -5, 7
    for fill in vc.COMPACT_FILLS:
        cand = vc.compact_input(X, Y, fill)
        ref, n = vc.ref_compact(cand, X, Y, ox, oy)
        c, cells, count = _dev(cand), _buf(2 * X * Y), _buf(1)
        L.call("mopa_vgi_compact_cells", L.ptr(c), X, Y, ox, oy, L.ptr(cells), L.ptr(count), L.stream())
        assert int(count[0]) == n, fill
        assert np.array_equal(cells[:2 * n].cpu().numpy().reshape(n, 2), ref), fill
        assert _untouched(cells, 2 * n) and _untouched(count, 1), fill
    cells, count = _buf(2 * X * Y), _buf(1)
    for bx, by in ((0, Y), (X, 0), (-X, Y)):
        _refused("mopa_vgi_compact_cells", L.ptr(c), bx, by, ox, oy, L.ptr(cells), L.ptr(count), L.stream())
        assert _untouched(cells) and _untouched(count)


# ------------------------------------------------------------------------------------------------ mopa_vgi_road_height
def _road(p, stride, n, vs, f, m, g, cell, out):
    L = _L()
    L.call("mopa_vgi_road_height", L.ptr(p), stride, n, float(np.float32(vs)), L.ptr(f), L.ptr(m), g["ox"], g["oy"], g["X"], g["Y"], g["zlo"],
           int(cell[0]), int(cell[1]), L.ptr(out), L.stream())


@pytest.mark.parametrize("n", vc.ROAD_SIZES)
def test_road_height_sum_and_count(n):
    """The lowest of two ground voxels; the non-ground points sharing it count; a column without ground gives (0, 0); z is a
    multiple of 2^-10, so the sum is exact: (sum, count) equal the reference and two calls give the same bits."""
    pts, flags, g = vc.ground_cloud(n)
    vs = g["vs"]
    first, _ = vc.ref_first_points(pts, vs, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], flags)
    g2d = vc.ref_ground_cells(first, flags, g["X"], g["Y"]).reshape(g["X"], g["Y"])
    some = (np.argwhere(g2d)[::29] + [g["ox"], g["oy"]]).tolist()
    f, m = _dev(first), _dev(flags)
    for stride in (3, 5):
        p = _dev(vc.pad_stride(pts, stride))
        for cell in list(vc.GROUND_CELLS.values()) + some:
            want = vc.ref_road_height(pts, vs, first, flags, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], cell)
            a, b = _buf(2, torch.float64), _buf(2, torch.float64)
            _road(p, stride, n, vs, f, m, g, cell, a)
            _road(p, stride, n, vs, f, m, g, cell, b)
            assert tuple(a[:2].tolist()) == want, (cell, stride)
            assert a[:2].cpu().numpy().tobytes() == b[:2].cpu().numpy().tobytes() and _untouched(a, 2) and _untouched(b, 2)
    if n >= 1023:
        assert vc.ref_road_height(pts, vs, first, flags, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], vc.GROUND_CELLS["late"]) == (0.0, 0.0)
        assert vc.ref_road_height(pts, vs, first, flags, g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], vc.GROUND_CELLS["two"])[1] > 300


def test_road_height_refuses_cells_outside_the_map_and_bad_arguments():
    L = _L()
    pts, flags, g = vc.ground_cloud(200)
    first, _ = vc.ref_first_points(pts, g["vs"], g["ox"], g["oy"], g["X"], g["Y"], g["zlo"], flags)
    p, f, m, out = _dev(pts), _dev(first), _dev(flags), _buf(2, torch.float64)
    ox, oy, X, Y = g["ox"], g["oy"], g["X"], g["Y"]
    good = dict(stride=3, n=200, vs=0.5, X=X, Y=Y, cell=(ox, oy))
    _road(p, 3, 200, 0.5, f, m, g, (ox + X - 1, oy + Y - 1), out)           # the last cell of the map is inside
    assert not _untouched(out, 0) and _untouched(out, 2)
    out = _buf(2, torch.float64)
    for bad in (dict(cell=(ox - 1, oy)), dict(cell=(ox + X, oy)), dict(cell=(ox, oy - 1)), dict(cell=(ox, oy + Y)), dict(n=0), dict(n=-1),
                dict(stride=2), dict(vs=0.0), dict(vs=float("nan")), dict(X=0), dict(Y=0)):
        a = dict(good, **bad)
        _refused("mopa_vgi_road_height", L.ptr(p), a["stride"], a["n"], a["vs"], L.ptr(f), L.ptr(m), ox, oy, a["X"], a["Y"], g["zlo"],
                 a["cell"][0], a["cell"][1], L.ptr(out), L.stream())
        assert _untouched(out), bad


# ------------------------------------------------------------------------------------------------ mopa_vgi_range_keep
@pytest.mark.parametrize("name", list(vc.range_cases()))
def test_range_keep_equals_the_oracle(name):
    """Two and three points of bit-equal depth in a pixel (the smallest index survives, scan or object), pixels with scan points
    only, a scan point in front of object points and behind one, no scan points / no object points, points above and below the
    field of view, the four axes with y = +0.0 and -0.0 behind the sensor, n = 1 and n = 257."""
    L = _L()
    c = vc.range_cases()[name]
    pts, n0, W, H = c["pts"], c["n_scan"], c["W"], c["H"]
    n = len(pts)
    ref = vc.ref_range_keep(pts, n0, c["fov_up"], c["fov_down"], W, H)
    if n0 < n:
        assert np.array_equal(ref, ovgi.range_keep(pts, np.arange(n) >= n0, c["fov_up"], c["fov_down"], W, H))
    p, keep = _dev(pts), _buf(n, torch.uint8)
    ws = _Ws(L.query("mopa_vgi_range_keep_workspace_bytes", n, W, H))
    L.call("mopa_vgi_range_keep", L.ptr(p), n, n0, c["fov_up"], c["fov_down"], W, H, L.ptr(keep), L.ptr(ws.t), ws.nbytes, L.stream())
    got = keep[:n].cpu().numpy()
    assert np.array_equal(got, ref.astype(np.uint8))
    for row, kept in c["expect"].items():
        assert bool(got[row]) == kept, row
    assert _untouched(keep, n) and ws.ok()
    if name in ("random_257", "one_object_point"):
        keep2, ws2 = _buf(n, torch.uint8), _Ws(ws.nbytes)
        good = dict(n=n, n0=n0, W=W, H=H, short=0)
        for bad in (dict(short=1), dict(n=0), dict(n=-3), dict(n0=-1), dict(n0=n + 1), dict(W=0), dict(H=0), dict(W=-16)):
            a = dict(good, **bad)
            _refused("mopa_vgi_range_keep", L.ptr(p), a["n"], a["n0"], c["fov_up"], c["fov_down"], a["W"], a["H"], L.ptr(keep2), L.ptr(ws2.t),
                     ws2.nbytes - a["short"], L.stream())
            assert _untouched(keep2) and ws2.clean(), bad


# ------------------------------------------------------------------------------------------------ mopa_voxelize_f64
def _voxelize(c, n=None, full_scale=None, transl=None, u="case", ws_short=0, out=None):
    L = _L()
    n = len(c["pts"]) if n is None else n
    p = _dev(c["pts"])
    k = None if c["keep_in"] is None else _dev(c["keep_in"])
    coords, keep = out if out is not None else (_buf(4 * len(c["pts"]), torch.int64), _buf(len(c["pts"]), torch.uint8))
    ws = _Ws(L.query("mopa_voxelize_f64_workspace_bytes"))
    u = c["u"] if isinstance(u, str) else u
    L.call("mopa_voxelize_f64", L.ptr(p), n, L.ptr(k), None if c["R"] is None else c["R"].ctypes.data, float(c["scale"]),
           c["full_scale"] if full_scale is None else full_scale, None if u is None else u.ctypes.data,
           int(c["u"] is not None) if transl is None else transl, c["batch"], L.ptr(coords), L.ptr(keep), L.ptr(ws.t), ws.nbytes - ws_short,
           L.stream())
    return coords, keep, ws


@pytest.mark.parametrize("name", list(vc.voxel_cases()))
def test_voxelize_f64_equals_the_restated_reference(name):
    """No rotation and flips (exact products); scaled coordinates of exactly k + 0.5 (ties to even, k < 0 and k > 0); keep_in
    NULL, partly zero (the extremes culled), all zero; translation with an extent below and above the field; coordinates of
    exactly 0 (in) and full_scale (out); the batch index in column 3; one seeded noisy rotation on random points."""
    c = vc.voxel_cases()[name]
    n = len(c["pts"])
    ref_coords, ref_keep = vc.ref_voxelize_f64(c["pts"], c["keep_in"], c["R"], c["scale"], c["full_scale"], c["u"], c["batch"])
    coords, keep, ws = _voxelize(c)
    got_keep, got = keep[:n].cpu().numpy(), coords[:4 * n].cpu().numpy().reshape(n, 4)
    assert np.array_equal(got_keep, ref_keep.astype(np.uint8))
    assert np.array_equal(got[ref_keep], ref_coords[ref_keep])
    assert (got[:, 3] == c["batch"]).all()
    kin = np.ones(n, bool) if c["keep_in"] is None else c["keep_in"] != 0
    if kin.any() and name != "noisy_rotation":      # rows that only the field filter culls still hold the reference's coordinates
        assert np.array_equal(got[kin], ref_coords[kin])
    assert _untouched(coords, 4 * n) and _untouched(keep, n) and ws.ok()


def test_voxelize_f64_refuses_bad_arguments():
    c = vc.voxel_cases()["translation_extent_below_field"]
    out = (_buf(4 * len(c["pts"]), torch.int64), _buf(len(c["pts"]), torch.uint8))
    for bad in (dict(u=None, transl=1), dict(n=0), dict(n=-1), dict(full_scale=0), dict(full_scale=-64), dict(ws_short=1)):
        with pytest.raises(RuntimeError):
            _voxelize(c, out=out, **bad)
        torch.cuda.synchronize()
        assert _untouched(out[0]) and _untouched(out[1]), bad
    coords, keep, ws = _voxelize(c, u=None, transl=0)          # without translation u may be NULL
    ref_coords, ref_keep = vc.ref_voxelize_f64(c["pts"], None, None, c["scale"], c["full_scale"], None, c["batch"])
    n = len(c["pts"])
    assert np.array_equal(keep[:n].cpu().numpy(), ref_keep.astype(np.uint8)) and np.array_equal(coords[:4 * n].cpu().numpy().reshape(n, 4), ref_coords)


# ------------------------------------------------------------------------------------------------ Python level
def test_free_cells_is_none_exactly_where_the_box_does_not_fit():
    """An object whose box is as wide as the map still has one column of cells; one cell wider, or taller than the slab, has none:
    free is None exactly where the oracle's free volume is empty."""
    from mopa_amd import vgi
    vs, sr, front = vc.MAPS["vs0.5_x"]
    pts, _ = vc.first_cloud(vs, sr, front, 300)
    m = vgi.OverlapMap(pts, vs, sr, -2.0, front)
    want_none = {"fits": False, "box_equals_the_map": False, "wider_than_the_map": True, "taller_than_the_slab": True,
                 "as_tall_as_the_slab": False}
    for name, (obj, z_max) in vc.free_cells_objects().items():
        o = ovgi.overlap_grid(pts, obj, vs, sr, -2.0, z_max, front)
        fc = m.free_cells(obj, z_max)
        assert (fc["free"] is None) == (o["free"].size == 0) == want_none[name], name
        assert np.array_equal(fc["box"], o["box"]) and np.array_equal(fc["extent"], o["extent"]) and np.array_equal(fc["offset"], o["offset"])
        if fc["free"] is not None:
            assert np.array_equal(fc["free"].cpu().numpy() != 0, o["free"]), name
        got = vgi.check_overlap(pts, obj, vs, sr, -2.0, z_max, front)
        want = ovgi.check_overlap(pts, obj, vs, sr, -2.0, z_max, front)
        assert (got is None) == (want is None) and (got is None or np.array_equal(got, want)), name
    assert int(m.status.item()) == 0


@pytest.mark.parametrize("vs", vc.OVERLAP_VOXEL_SIZES)
def test_check_overlap_equals_the_oracle_at_any_voxel_size(vs):
    """0.5 and 0.25 (both quotients exact) and 0.2 and 0.3, where a voxel's representative is the first point of its FLOAT64 voxel
    and is marked at its FLOAT32 floor: the cloud holds the two-point case [[1.3, ..], [1.4, ..]] in both orders and 700 points
    within a float32 ulp of k * vs; the object has such a pair too (its box follows its representatives)."""
    from mopa_amd import vgi
    scan, obj = vc.overlap_cloud(vs)
    g = vc.map_geometry(vs, vc.OVERLAP_RANGE, "x")
    o = ovgi.overlap_grid(scan, obj, vs, vc.OVERLAP_RANGE, -2.0, None, "x")
    m = vgi.OverlapMap(scan, vs, vc.OVERLAP_RANGE, -2.0, "x")
    assert m.by_reps == (vs in (0.2, 0.3))
    z0 = int(np.floor(-2.0 / vs)) - g["zlo"]
    vol = m.first.cpu().numpy().reshape(g["X"], g["Y"], vc.ZR)
    assert np.array_equal(vol[:, :, z0:z0 + o["grid"].shape[2]] != INT_MAX, o["grid"] != 0)
    fc = m.free_cells(obj)
    assert np.array_equal(fc["box"], o["box"]) and np.array_equal(fc["free"].cpu().numpy() != 0, o["free"])
    want = ovgi.check_overlap(scan, obj, vs, vc.OVERLAP_RANGE, -2.0, None, "x")
    got = vgi.check_overlap(scan, obj, vs, vc.OVERLAP_RANGE, -2.0, None, "x")
    assert want is not None and got is not None and got.dtype == np.float64 and np.array_equal(got, want)
    for pair in (vc.PAIR, vc.PAIR[::-1].copy()):               # the two-point case alone, at the reference's default arguments
        obj2 = np.array([[5, 5, 0], [5.1, 5.1, 0.1]])
        assert np.array_equal(vgi.check_overlap(pair, obj2, vs, (2.5, 2.5), -2.0, None, "x"), ovgi.check_overlap(pair, obj2, vs, (2.5, 2.5), -2.0, None, "x"))
