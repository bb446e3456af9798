"""Shared by tests/test_spconv_picks_host.py (no GPU) and tests/test_gpu_spconv_kernels.py: the value mopa_spconv_fwd_kernel returns
(csrc/sprun_pack.h), the enumeration of the forward dispatch rules of csrc/spconv.hip and csrc/sprun.hip over every threshold, the
witness table it yields -- for every distinct kernel instantiation one (entry, K, stated rows, cin, cout, flags) that selects it --
and the small geometries the kernels are run on."""
import functools
import itertools

import numpy as np

ENTRIES = ("mopa_spconv_fwd", "mopa_spconv_fwd_grouped", "mopa_spconv_fwd_run")
ROWS_8_SCANS = (257465, 193135, 103554, 49022, 19312, 6789, 2330)   # active rows per level of 8 scans (tests/test_spconv_plan.py)
STEM, FWD, BLK, PIPE, T4, RUN = 1, 2, 3, 4, 5, 6
PIPE_MU = {1: 40, 2: 32, 3: 40, 4: 28}
UNALIGNED_PAIRS = ((3, 20), (20, 16), (24, 40))
RTOL, ATOL = 1e-4, 2e-5   # the project's forward bounds (tests/test_gpu_3d.py): atol x max(1, max|ref|)


def parts(pick):
    return dict(family=pick & 15, ntw=(pick >> 4) & 15, nk=(pick >> 8) & 15, d=(pick >> 12) & 15, nwv=(pick >> 16) & 7,
                flag=(pick >> 19) & 1, osplit=(pick >> 20) & 15, rg=(pick >> 24) & 3)


def kernel_name(pick):
    """The instantiation a pick launches, as csrc/spconv.hip / csrc/sprun.hip spell it (a block-kernel launch with osplit > 1 also
    runs k_sum_partials over that many partial copies: another path through the launcher, so it is part of the name)."""
    p = parts(pick)
    b = ("false", "true")[p["flag"]]
    f = p["family"]
    if f == STEM:
        return f"k_spconv_stem<{p['ntw']},{16 * p['nk']}>"
    if f == FWD:
        return f"k_spconv_fwd<{p['ntw']},{p['nk']},{b}>"
    if f == BLK:
        return f"k_spconv_blk<{p['ntw']},{p['nk']},{b}>" + (f" osplit {p['osplit']}" if p["osplit"] > 1 else "")
    if f == PIPE:
        return f"k_spconv_pipe<{p['ntw']},{p['d']},{PIPE_MU[p['ntw']]}>"
    if f == T4:
        return f"k_spconv_t4<{p['ntw']},{p['nk']},{p['d']},{b},{p['nwv']}>"
    if f == RUN:
        return f"k_spconv_run<{p['ntw']},{p['rg']},{b}>"
    raise ValueError(hex(pick))


def stated(rows):
    """The bits of w_flip that state a table size: `rows` (a multiple of 64) as 64-row tiles in bits 8-30; 0 states nothing."""
    assert rows % 64 == 0 and 0 <= rows // 64 < 1 << 23
    return (rows // 64) << 8


def pick_of(entry, K, rows, cin, cout, ld_in=None, w_flip=0, has_ws=0, one=0):
    from mopa_amd import _lib
    return int(_lib.load().mopa_spconv_fwd_kernel(entry, K, rows, cin, cout, cin if ld_in is None else ld_in, w_flip, has_ws, one))


# ---- the enumeration
def channel_pairs():
    from test_spconv_plan import channel_pairs as network_pairs
    mult16 = [(a, b) for a in range(16, 225, 16) for b in range(16, 225, 16)]
    return sorted(set(mult16) | set(network_pairs()) | set(UNALIGNED_PAIRS), key=lambda p: (p[0] + p[1], p))


def threshold_rows(cout):
    """Rows just under, at and over every table size at which a rule of the forward dispatch changes its answer for `cout` columns:
    256 / 768 / 800 / 1,024 / 1,500 tiles and their quotients by the column groups per tile nt / w (packed_plan, fwd_plan, the > 800
    test), 512 four-tile blocks (blk_plan), the block counts at which blk_osplit steps (3,072 / s), the row counts at which
    k_spconv_run's items double (rg), and the levels of 8 scans."""
    nt = (cout + 15) // 16
    ms = sorted({nt // c for c in (1, 2, 3, 4) if nt % c == 0} | {-(-nt // c) for c in (1, 2, 4)})
    tiles = set()
    for base in (256, 512, 768, 800, 1024, 1500) + tuple(-(-3072 // s) for s in range(1, 10)):
        for m in ms:
            t = -(-base // m)
            tiles |= {t, 4 * t, 4 * (t - 1)}
    rows = set(ROWS_8_SCANS) | {14563, 14564, 52428, 52429, 131071, 131072}
    tiles |= {r // 64 + i for r in rows for i in (0, 1)}   # (whole tiles on both sides: what a stated size can name)
    for t in tiles:
        if t > 0:
            rows |= {64 * (t - 1), 64 * (t - 1) + 1, 64 * t, 64 * t + 1, 64 * (t + 1)}
    return sorted(r for r in rows if r > 0)


@functools.lru_cache(maxsize=None)
def enumerate_picks():
    """-> {(entry, K, rows, cin, cout, w_flip bit 1, has_ws, one_rule_per_row): pick} over the whole grid; refusals (< 0) included."""
    out = {}
    for cin, cout in channel_pairs():
        for K, rows in itertools.product((8, 27), threshold_rows(cout)):
            out[(0, K, rows, cin, cout, 0, 0, 0)] = pick_of(0, K, rows, cin, cout)
            for packed, ws in itertools.product((0, 1), (0, 1)):
                out[(1, K, rows, cin, cout, packed, ws, 0)] = pick_of(1, K, rows, cin, cout, w_flip=2 * packed, has_ws=ws)
            for one in ((0, 1) if K == 8 else (0,)):
                out[(2, K, rows, cin, cout, 0, 1, one)] = pick_of(2, K, rows, cin, cout, has_ws=1, one=one)
    return out


@functools.lru_cache(maxsize=None)
def witness_table():
    """-> {(entry, kernel name): (entry, K, stated rows, cin, cout, packed, has_ws, one)}: for every instantiation the enumeration
    reaches, the case with the fewest channels (then the shortest table) that selects it through the stated size alone."""
    picks = enumerate_picks()
    table, every = {}, set()
    for case, pick in sorted(picks.items(), key=lambda kv: (kv[0][3] + kv[0][4], kv[0][2], kv[0])):
        if pick < 0:
            continue
        key = (case[0], case[1], kernel_name(pick))
        every.add(key)
        if case[2] % 64 == 0 and key not in table:
            table[key] = case
    assert set(table) == every, sorted(every - set(table))   # the stated size reaches everything the rules reach
    return table


# ---- the geometries (voxel coordinates with a batch column; built with Geometry3D / oracle.scn3d.Geometry by the tests)
def _mixed_points():
    cube = list(itertools.product(range(8, 14), repeat=3))
    isolated = list(itertools.product(range(20, 60, 4), [2, 6, 10], [30, 34, 38, 42]))
    line = [(x, 50, 50) for x in range(3, 60)]
    return np.asarray(cube + isolated + line, np.int64)


def geometry_coords(name):
    """-> (coords (N, 4) int64, levels, full_scale)"""
    def batch(p, b):
        return np.concatenate([p, np.full((len(p), 1), b, np.int64)], 1)
    if name == "mixed":
        return batch(_mixed_points(), 0), 3, 64
    if name == "block8":
        return batch(np.asarray(list(itertools.product(range(8, 16), repeat=3)), np.int64), 0), 3, 64
    if name == "one":
        return batch(np.asarray([(5, 5, 5)], np.int64), 0), 2, 64
    if name == "two":
        return np.concatenate([batch(_mixed_points(), 0), batch(_mixed_points(), 1)]), 3, 64
    raise KeyError(name)


GEOMETRIES = ("mixed", "block8", "one", "two")
# rows per level and the groups per 64-row tile the oracle's tables give (asserted: a change of the generator cannot hollow the cases out)
EXPECT_ROWS = {"mixed": (393, 176, 143), "block8": (512, 64, 8), "one": (1, 1), "two": (786, 352, 286)}
EXPECT_GROUPS = {("mixed", "nbr27", 0): (84, 96, 92, 34, 4, 10, 3), ("mixed", "ch", 0): (18, 4, 5), ("mixed", "up", 0): (8, 8, 8, 7, 4, 5, 2),
                 ("mixed", "nbr27", 2): (70, 75, 3), ("block8", "ch", 0): (32,), ("block8", "nbr27", 1): (74,), ("one", "nbr27", 0): (1,)}


def tile_groups(nbr):
    """Groups per 64-row tile of a rule table: every (tile, offset) with n rules holds ceil(n / 16) groups of 16 (csrc/spconv.hip)."""
    nbr = np.asarray(nbr)
    K, A = nbr.shape
    return tuple(int(sum(-(-int((nbr[o, t:t + 64] >= 0).sum()) // 16) for o in range(K))) for t in range(0, A, 64))


@functools.lru_cache(maxsize=None)
def oracle_geometry(name):
    from oracle import scn3d
    coords, levels, fs = geometry_coords(name)
    return scn3d.Geometry(coords, levels, fs)


def tables_of(name, K, one=None):
    """The (kind, level, flip) launches of a geometry for a K-offset witness: the finest 27-offset table plain and with mirrored
    offsets and the deeper tables the cases were chosen for, or the stride-2 convolution and deconvolution tables (`one`: only
    those with / without exactly one rule per row)."""
    if K == 27:
        return [("nbr27", 0, 0), ("nbr27", 0, 1)] + {"mixed": [("nbr27", 2, 0)], "block8": [("nbr27", 1, 1)]}.get(name, [])
    kinds = ("ch", "up") if one is None else (("up",) if one else ("ch",))
    return [(k, l, 0) for k in kinds for l in ((0, 1) if name == "mixed" else (0,))]


def inputs(K, A_in, cin, cout, seed):
    """Standard-normal rows and 0.2 x standard-normal weights (float32), as tests/test_gpu_3d.py draws them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((A_in, cin), dtype=np.float32), rng.standard_normal((K, cin, cout), dtype=np.float32) * np.float32(0.2)


def rows_in(o, kind, level):
    return o.num_active[level + 1] if kind == "up" else o.num_active[level]


@functools.lru_cache(maxsize=None)
def reference(name, kind, level, flip, cin, cout):
    """-> (x, w float32 numpy, oracle.scn3d.sparse_conv of them in float64 as numpy): computed once per case and shared."""
    import torch
    from oracle import scn3d
    o = oracle_geometry(name)
    tab = getattr(o, kind)[level]
    x, w = inputs(tab.shape[0], rows_in(o, kind, level), cin, cout, 7919 * cin + 31 * cout + 3 * level + len(kind))
    wd = torch.from_numpy(w).double()
    ref = scn3d.sparse_conv(torch.from_numpy(x).double(), tab, wd.flip(0) if flip else wd)
    return x, w, ref.numpy()


def bound(ref):
    """The absolute part of the GPU bound for a result: |got - ref| <= ATOL max(1, max|ref|) + RTOL |ref|."""
    return ATOL * max(1.0, float(np.abs(ref).max()))


# ---- the device side (imported by the GPU test and by tests/_spconv_path_worker.py)
SENTINEL = -777.0
GUARD_ROWS = 64    # sentinel rows behind row A_out of the output buffer
COL0 = 4           # the slices start at a 16-byte-aligned column of a wider buffer


def slice_ld(c):
    return 4 * -(-c // 4) + 2 * COL0


class Bench3D:
    """The geometries on the device (checked against the oracle's), the tables' rulebooks, and per case the inputs, the float64
    reference and the dense-table kernel's result on the device -- each built once and left unchanged."""

    def __init__(self):
        import torch
        from mopa_amd.sparse3d import Geometry3D
        self.g, self._dev, self._runs = {}, {}, {}
        for name in GEOMETRIES:
            coords, levels, fs = geometry_coords(name)
            self.g[name] = Geometry3D(torch.from_numpy(coords), levels, fs, "cuda")

    def table(self, name, kind, level):
        return getattr(self.g[name], kind)[level]

    def runs(self, name, kind, level):
        """(run-major rulebook, one-rule-per-row fact): the geometry's, or -- the stride-2 convolution tables get none -- built here."""
        import torch
        from mopa_amd._lib import call, query, stream
        tab = self.table(name, kind, level)
        r = self.g[name].runs(tab)
        if r is None:
            r = self._runs.get((name, kind, level))
        if r is None:
            K, A = tab.shape
            buf = torch.empty(query("mopa_rulebook_runs_bytes", K, A) // 4, dtype=torch.int32, device="cuda")
            desc = np.asarray([(tab.data_ptr(), K, A, buf.data_ptr())], dtype=np.int64)
            call("mopa_rulebook_runs_build_batched", desc.ctypes.data, 1, stream())
            r = self._runs[(name, kind, level)] = (buf, 0)
        return r

    def case(self, name, kind, level, flip, cin, cout):
        """-> (input buffer with NaN around the slice, weight, reference float64, allowed error per element, dense-table result)"""
        import torch
        from mopa_amd._lib import call, ptr, stream
        key = (name, kind, level, flip, cin, cout)
        hit = self._dev.get(key)
        if hit is None:
            x, w, ref = reference(*key)
            xin = torch.full((x.shape[0], slice_ld(cin)), float("nan"), device="cuda")
            xin[:, COL0:COL0 + cin] = torch.from_numpy(x).cuda()
            wd, refd = torch.from_numpy(w).cuda(), torch.from_numpy(ref).cuda()
            allowed = bound(ref) + RTOL * refd.abs()
            dense = None
            if cin <= 192:   # the dense-table kernel with the rules' own choice: what the other kernels' bits are compared with
                tab = self.table(name, kind, level)
                buf = torch.full((tab.shape[1], slice_ld(cout)), SENTINEL, device="cuda")
                call("mopa_spconv_fwd", ptr(tab), tab.shape[0], tab.shape[1], ptr(xin, COL0), xin.shape[1], cin, ptr(wd), cout, flip,
                     ptr(buf, COL0), buf.shape[1], stream())
                dense = buf[:, COL0:COL0 + cout].clone()
            hit = self._dev[key] = (xin, wd, refd, allowed, dense, max(1.0, float(np.abs(ref).max())))
        return hit

    def launch(self, case, name, kind, level, flip, transposed=False, out=None):
        """One launch of a witness (entry, K, stated rows, cin, cout, packed, has_ws, one) through the C ABI on a table of a geometry,
        the stated size in w_flip.  -> (kernel name the query gives for this very call, output buffer)."""
        import torch
        from mopa_amd._lib import call, ptr, query, stream
        entry, K, rows, cin, cout, packed, has_ws, one = case
        tab = self.table(name, kind, level)
        assert tab.shape[0] == K
        A_out = tab.shape[1]
        xin, wd, _, _, _, _ = self.case(name, kind, level, flip, cin, cout)
        wf = stated(rows) | flip | 2 * packed
        st = stream()
        layer_w = wd.transpose(1, 2).contiguous() if transposed else wd   # backward-data: the layer's weight is [K][cout][cin]
        wshape = (K, cout, cin) if transposed else (K, cin, cout)
        if entry == 2:
            wk = torch.empty_like(wd)
            call("mopa_spconv_run_pack_weight", ptr(layer_w), *wshape, int(transposed), ptr(wk), st)
        elif packed:
            ntw = query("mopa_spconv_grouped_wants_packed", K, rows or A_out, cin, cout)
            assert ntw > 0, case
            wk = torch.empty_like(wd)
            call("mopa_spconv_pack_weight", ptr(layer_w), *wshape, int(transposed), ntw, ptr(wk), st)
        elif transposed:
            wk = torch.empty_like(wd)
            call("mopa_spconv_transpose_weight", ptr(layer_w), *wshape, ptr(wk), st)
        else:
            wk = wd
        ld_in, ld_out = xin.shape[1], slice_ld(cout)
        pick = pick_of(entry, K, A_out, cin, cout, ld_in, wf, has_ws, one)
        assert pick > 0, (case, pick)
        if out is None:
            out = torch.full((A_out + GUARD_ROWS, ld_out), SENTINEL, device="cuda")
        if entry == 0:
            call("mopa_spconv_fwd", ptr(tab), K, A_out, ptr(xin, COL0), ld_in, cin, ptr(wk), cout, wf, ptr(out, COL0), ld_out, st)
        elif entry == 1:
            gs, go, gi, gout = self.g[name].rulebook(tab)
            ws = torch.empty(query("mopa_spconv_grouped_workspace_bytes", K, A_out, cout) // 4, device="cuda") if has_ws else None
            call("mopa_spconv_fwd_grouped", ptr(gs), ptr(go), ptr(gi), ptr(gout), K, A_out, ptr(xin, COL0), ld_in, cin, ptr(wk), cout, wf,
                 ptr(out, COL0), ld_out, ptr(ws), 0 if ws is None else 4 * ws.numel(), st)
        else:
            buf, t_one = self.runs(name, kind, level)
            assert t_one == one, (case, kind)
            ws = None if one else torch.empty(query("mopa_spconv_run_workspace_bytes", K, A_out, cout) // 4, device="cuda")
            call("mopa_spconv_fwd_run", ptr(buf), K, A_out, ptr(xin, COL0), ld_in, cin, ptr(wk), cout, wf, ptr(out, COL0), ld_out, one,
                 ptr(ws), 0 if ws is None else 4 * ws.numel(), st)
        return kernel_name(pick), out

    def measure(self, case, name, kind, level, flip, transposed=False):
        """Two launches of a witness.  -> (kernel name, device vector [worst error / allowed error, worst error / max(1, max|ref|), every
        sentinel untouched, the second launch's bits equal the first's, the bits equal the dense-table kernel's (-1: not compared)])."""
        import torch
        cin, cout = case[3], case[4]
        _, _, refd, allowed, dense, scale = self.case(name, kind, level, flip, cin, cout)
        kname, out = self.launch(case, name, kind, level, flip, transposed)
        _, out2 = self.launch(case, name, kind, level, flip, transposed)
        A = refd.shape[0]
        got = out[:A, COL0:COL0 + cout]
        err = (got.double() - refd).abs()
        ratio = torch.nan_to_num(err / allowed, nan=float("inf")).max()
        quiet = (out[:, :COL0] == SENTINEL).all() & (out[:, COL0 + cout:] == SENTINEL).all() & (out[A:] == SENTINEL).all()
        same = (got == dense).all().double() if dense is not None else torch.tensor(-1.0, device="cuda", dtype=torch.float64)
        return kname, torch.stack([ratio, torch.nan_to_num(err, nan=float("inf")).max() / scale, quiet.double(),
                                   (out == out2).all().double(), same])
