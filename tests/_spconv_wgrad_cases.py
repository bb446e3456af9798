"""Shared by tests/test_spconv_wgrad_picks_host.py (no GPU) and tests/test_gpu_spconv_wgrad_kernels.py: the value
mopa_spconv_wgrad_kernel returns (csrc/sprun_pack.h, WGK), the enumeration of the weight-gradient dispatch of csrc/spconv.hip
(pick_wgrad) and csrc/sprun.hip (wgr_pick) over every threshold, the witness table it yields -- for every kernel instantiation the
rules reach one (entry, K, stated rows, cin, cout, variant, one_rule_per_row) that selects it -- the float64 reference
dW[o] = X[in_rows(o)]^T G[out_rows(o)], the census of the kernel edges the launched cases contain, and the device-side plumbing."""
import ctypes
import functools
import itertools
import math

import numpy as np

import _spconv_cases as C

ENTRIES = ("mopa_spconv_bwd_weight", "mopa_spconv_bwd_weight_run")
ROWS_8_SCANS = C.ROWS_8_SCANS
STEM, SIMPLE, PIPE, RUN = 1, 2, 3, 4
RTOL, ATOL = 2e-4, 5e-5   # the project's weight-gradient bound (tests/test_gpu_3d.py): atol x max(1, max|ref|)
I_CHUNKS, I_RPC, I_S, I_PIECES, I_WS, I_LDS, I_BLOCKS = range(7)
WG2_CAP, WGR_TS, RUN_PAD = 1024, 32, 128
stated = C.stated   # the same bits in `accumulate` as in w_flip: 64-row tiles in bits 8-30

# How a call's operands lie in memory: (ld_in - cin, ld_dout - cout, low address bits of in, of dout, of ws).
# Table entry: 0 plain; 1 / 2 odd row strides (rows 4-byte aligned only; the stem needs ld_dout % 4 == 0); 3 / 4 `in` / `dout` at a
# 4-byte boundary (4: the stem shape falls to k_spconv_wgrad<1,1>); 5 `in` at a 2-byte boundary (query only: the simple kernel);
# 6 / 7 a row stride below the channel count (refused); 8 channel slices of buffers eight floats wider, at a 16-byte-aligned column.
TABLE_VARIANTS = ((0, 0, 0, 0, 0), (3, 0, 0, 0, 0), (0, 2, 0, 0, 0), (8, 8, 4, 0, 0), (8, 8, 0, 4, 0), (0, 0, 2, 0, 0), (-1, 0, 0, 0, 0),
                  (0, -1, 0, 0, 0), (8, 8, 0, 0, 0))
# Run entry: 0 plain; 1 slices of wider buffers; 2 / 3 ld % 4 != 0; 4 / 5 / 6 a pointer off the 16-byte grid; 7 ld_dout < cout.
RUN_VARIANTS = ((0, 0, 0, 0, 0), (8, 8, 0, 0, 0), (2, 0, 0, 0, 0), (0, 3, 0, 0, 0), (0, 0, 4, 0, 0), (0, 0, 0, 8, 0), (0, 0, 0, 0, 4),
                (0, -4, 0, 0, 0))
SLICED = {0: 8, 1: 1}   # per entry point: the layout every witness is launched in (ld = C + 8, the slice at column COL0, NaN around it)


def sliced(case):
    """The case with its operands as channel slices of wider buffers (a case that already has a layout of its own keeps it)."""
    return case if case[5] else case[:5] + (SLICED[case[0]],) + case[6:]


def parts(pick):
    return dict(family=pick & 15, mu=(pick >> 4) & 15, nt=(pick >> 8) & 15, d=(pick >> 12) & 15, nwv=(pick >> 16) & 7)


def kernel_name(pick):
    p = parts(pick)
    f = p["family"]
    if f == STEM:
        return "k_spconv_stem_wgrad<16>"
    if f == SIMPLE:
        return f"k_spconv_wgrad<{p['mu']},{p['nt']}>"
    if f == PIPE:
        return f"k_spconv_wgrad2<{p['mu']},{p['nt']},{p['d']},{p['nwv']}>"
    if f == RUN:
        return f"k_wgrad_run<{p['mu']},{p['nt']}>"
    raise ValueError(hex(pick))


_INFO = (ctypes.c_int64 * 8)()


def ask(entry, K, rows, cin, cout, variant=0, one=0, accumulate=0):
    """-> (pick or error code, (chunks, rows per chunk, S, pieces, workspace bytes, LDS bytes, blocks)) of mopa_spconv_wgrad_kernel"""
    from mopa_amd import _lib
    dli, dlo, li, lo, lw = (TABLE_VARIANTS, RUN_VARIANTS)[entry][variant]
    rc = int(_lib.load().mopa_spconv_wgrad_kernel(entry, K, rows, cin, cout, cin + dli, cout + dlo, accumulate, li | lo << 4 | lw << 8,
                                                  ctypes.addressof(_INFO), one))
    return rc, tuple(_INFO[:7])


# ---- the enumeration
def ragged_pairs():
    """Channel pairs that are no multiples of 16 and reach all 28 (MU, NT) of k_spconv_wgrad: ragged in cin only, in cout only, in both."""
    cins, couts = (15, 31, 47, 63, 80), (13, 16, 29, 45, 61, 77, 93, 109)
    return [(a, b) for a in cins for b in couts if a % 16 or b % 16] + [(a, 13) for a in (16, 32, 48, 64)] + [(1, 16), (3, 20), (16, 1)]


# beyond the grid: 48 x 7 input channels in one block per seven (three chunks on a table of 3,000 rows), and the widest pair
EXTRA_PAIRS = ((336, 96), (336, 112), (448, 80))


def channel_pairs():
    from test_spconv_plan import channel_pairs as network_pairs
    mult16 = [(a, b) for a in range(16, 257, 16) for b in range(16, 113, 16)]
    return sorted(set(mult16) | set(network_pairs()) | set(ragged_pairs()) | set(EXTRA_PAIRS), key=lambda p: (p[0] + p[1], p))


def cdiv(a, b):
    return -(-a // b)


def raw_piece(K, one, rows, ncu=256):
    """The piece size of k_wgrad_run before its clamps (csrc/sprun.hip wgr_plan)."""
    est = rows if one else 9 * rows if K == 27 else 5 * rows // 2
    s = est // (3 * ncu) if one else int(1.2 * math.sqrt(est))
    return cdiv(s, WGR_TS) * WGR_TS


def first_rows(pred, hi=1 << 29):
    """The smallest row count at which a monotone predicate holds (None: never below `hi`)."""
    if not pred(hi):
        return None
    lo = 1
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid + 1, hi)
    return lo


@functools.lru_cache(maxsize=None)
def threshold_rows(K, cin, cout):
    """Rows just under, at and over every table size at which a rule of the two dispatches changes its answer for this shape: 4,096
    rows (the wave target), the chunk counts at which K x chunks x mblocks passes 4,200 blocks, 256 rows per chunk against every wave
    target, against the 32 MB slab cap and against 2,048 chunks, 512 stem blocks, the piece sizes 128 and 1,024, the first table
    whose slabs pass 128 MiB, rows x ld = 2^32 for both operands at both strides, the levels of 8 scans -- and the whole 64-row
    tiles on both sides of each, which is what a stated size can name."""
    mt = cdiv(cin, 16)
    mu = next(c for c in (4, 3, 2, 1) if mt % c == 0)
    per = K * (mt // mu)
    rows = set(ROWS_8_SCANS) | {1, 63, 64, 65, 393, 4095, 4096, 4097, 256 * 512, 256 * 2048}
    limit = 4200 // per
    chunk_counts = {limit - 1, limit, limit + 1, limit + 2, 2048, (32 << 20) // (K * cin * cout * 4) + 1}
    chunk_counts |= {cdiv(w, per) for w in (512, 2048, 4096, 16384)}
    for c in chunk_counts:
        if c > 0:
            rows |= {256 * c, 256 * (c + 1), 256 * c + 192}
    for one in (0, 1):
        for s in (160, 1024, 1056):
            rows.add(first_rows(lambda r: raw_piece(K, one, r) >= s))
        bound = (lambda r: r + K * RUN_PAD) if one else (lambda r: cdiv(K * r + K * RUN_PAD, RUN_PAD) * RUN_PAD)
        rows.add(first_rows(lambda r: (bound(r) // min(max(raw_piece(K, one, r), 128), 1024) + K) * cin * cout * 4 > 128 << 20, 1 << 27))
    for ld in (cout, cout + 2, cout + 8, 8 * cin, 8 * (cin + 3), 8 * (cin + 8)):
        rows.add(cdiv(1 << 32, ld))
    rows.discard(None)
    out = set()
    for r in rows:
        t = r // 64
        out |= {r - 1, r, r + 1, 64 * (t - 1), 64 * t, 64 * (t + 1), 64 * (t + 2)}
    return sorted(r for r in out if 0 < r < 1 << 31)


@functools.lru_cache(maxsize=None)
def enumerate_picks(candidates_only=False):
    """-> {(entry, K, rows, cin, cout, variant, one_rule_per_row): (pick, info)} over the whole grid; refusals (pick < 0) included.
    candidates_only: just the cases a witness is taken from -- whole 64-row tiles, the plain layout (a fifth of the work; the host
    test holds the witness table against the whole grid)."""
    out = {}
    for cin, cout in channel_pairs():
        for K in (8, 27):
            every = threshold_rows(K, cin, cout)
            thin = set(every[::4]) | {r for r in every if r >= 1000000}   # the layouts other than the plain one: every fourth size, and all around 2^32 / ld
            if candidates_only:
                every, thin = [r for r in every if r % 64 == 0 and r < 1 << 29], ()
            for rows in every:
                for v in range(len(TABLE_VARIANTS) if rows in thin else 1):
                    out[(0, K, rows, cin, cout, v, 0)] = ask(0, K, rows, cin, cout, v)
                for v in range(len(RUN_VARIANTS) if rows in thin else 1):
                    for one in ((0, 1) if K == 8 else (0,)):
                        out[(1, K, rows, cin, cout, v, one)] = ask(1, K, rows, cin, cout, v, one)
    return out


def witness_key(case, pick):
    return (case[0], case[1], case[6], kernel_name(pick))


@functools.lru_cache(maxsize=None)
def witness_table():
    """-> {(entry, K, one_rule_per_row, kernel name): case}: for every instantiation, the case of the plain layout with the fewest
    channels (then the shortest table) that selects it through a stated size alone.  (That these are all the instantiations the
    rules reach, over every layout and row count: tests/test_spconv_wgrad_picks_host.py.)"""
    table = {}
    for case, (pick, _) in sorted(enumerate_picks(True).items(), key=lambda kv: (kv[0][3] + kv[0][4], kv[0][2], kv[0])):
        if pick > 0:
            table.setdefault(witness_key(case, pick), case)
    return table


# Launched beside the witnesses (same assertions): what the edge census needs and the witness rule (fewest channels) leaves out.
#   more than one Cin block per offset and chunk; a list of more than 1,024 rules (one wave per 1,152 rows of `cube15`); all four
#   wave slots of k_wgrad_run full, LDS above 64 KB; every MU of k_wgrad_run with no empty slot
EXTRAS = ((0, 27, 64 * 100, 80, 32, 0, 0), (0, 27, 64 * 100, 128, 48, 1, 0), (0, 8, 64 * 100, 160, 16, 0, 0), (0, 27, 64 * 100, 336, 96, 0, 0),
          (0, 27, 0, 336, 96, 0, 0), (0, 27, 0, 64, 64, 3, 0), (0, 27, 64 * 100, 31, 29, 3, 0),
          (1, 27, 0, 256, 112, 1, 0), (1, 8, 0, 224, 16, 0, 1), (1, 27, 64 * 2000, 64, 32, 0, 0), (1, 27, 0, 128, 48, 1, 0),
          (1, 8, 64 * 4000, 192, 64, 1, 1))


# ---- the geometries and tables
GEOMETRIES = C.GEOMETRIES + ("cube15",)


def geometry_coords(name):
    if name == "cube15":   # 3,375 rows, every interior row with all 27 rules: chunks of more than 1,024 rules per offset
        p = np.asarray(list(itertools.product(range(4, 19), repeat=3)), np.int64)
        return np.concatenate([p, np.zeros((len(p), 1), np.int64)], 1), 2, 32
    return C.geometry_coords(name)


@functools.lru_cache(maxsize=None)
def oracle_geometry(name):
    from oracle import scn3d
    coords, levels, fs = geometry_coords(name)
    return scn3d.Geometry(coords, levels, fs)


def tables_of(name, K):
    """(kind, level) of a geometry's tables for a K-offset case: the 27-offset table, or the stride-2 convolution and deconvolution."""
    if name == "cube15":
        return [("nbr27", 0)] if K == 27 else []
    if K == 27:
        return [("nbr27", 0)] + {"mixed": [("nbr27", 2)], "block8": [("nbr27", 1)]}.get(name, [])
    return [(k, l) for k in ("ch", "up") for l in ((0, 1) if name == "mixed" else (0,))]


def launches_of(case):
    """-> [(geometry, kind, level, swap)] a case is launched on.  The run entry takes a table with its own one_rule_per_row; with
    swap = 1 it reads the deconvolution table's lists for the stride-2 convolution's gradient.  `cube15` only for the wide extras."""
    entry, K, rows, cin, cout, v, one = case
    out = []
    for g in GEOMETRIES:
        if g == "cube15" and cin < 336:
            continue
        for kind, level in tables_of(g, K):
            if entry == 0:
                out.append((g, kind, level, 0))
            elif K == 27 or (kind == "up") == bool(one):
                out.append((g, kind, level, 0))
                if one:
                    out.append((g, kind, level, 1))
    return out


def table_np(name, kind, level):
    return np.asarray(getattr(oracle_geometry(name), kind)[level])


def rows_in(name, kind, level):
    o = oracle_geometry(name)
    return o.num_active[level + 1] if kind == "up" else o.num_active[level]


def inputs(A_in, A_out, cin, cout, seed):
    """Standard-normal rows and output gradients (float32), as tests/test_gpu_3d.py draws them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((A_in, cin), dtype=np.float32), rng.standard_normal((A_out, cout), dtype=np.float32)


def wgrad64(x, g, nbr):
    """dW[o] = X[in_rows(o)]^T G[out_rows(o)] in float64"""
    x, g = x.astype(np.float64), g.astype(np.float64)
    dw = np.zeros((nbr.shape[0], x.shape[1], g.shape[1]))
    for o in range(nbr.shape[0]):
        rows = np.flatnonzero(nbr[o] >= 0)
        if len(rows):
            dw[o] = x[nbr[o, rows]].T @ g[rows]
    return dw


@functools.lru_cache(maxsize=None)
def reference(name, kind, level, cin, cout):
    """-> (x, g float32, dW float64) on the table's own rules: computed once per (table, cin, cout) and shared, never written to."""
    nbr = table_np(name, kind, level)
    x, g = inputs(rows_in(name, kind, level), nbr.shape[1], cin, cout, 7919 * cin + 31 * cout + 3 * level + len(kind) + 101 * len(name))
    ref = wgrad64(x, g, nbr)
    for a in (x, g, ref):
        a.setflags(write=False)
    return x, g, ref


def allowed(ref):
    return ATOL * max(1.0, float(np.abs(ref).max())) + RTOL * np.abs(ref)


def launched_cases():
    return sorted(set(witness_table().values()) | set(EXTRAS))


# ---- the census of kernel edges (host arithmetic on the tables and the plans the query returns)
def plan_of(case, A_out):
    entry, K, rows, cin, cout, v, one = case
    pick, info = ask(entry, K, A_out, cin, cout, v, one, stated(rows))
    assert pick > 0, (case, A_out, pick)
    return pick, info


def wave_rule_counts(nbr, rpc, nwv):
    """-> (n[o, chunk, wave], empty[chunk, wave]): rules in every wave's row range of a k_spconv_wgrad2 launch, and which ranges
    start at or past their chunk's end."""
    K, A = nbr.shape
    cum = np.concatenate([np.zeros((K, 1), np.int64), np.cumsum(nbr >= 0, 1)], 1)
    nchunks = cdiv(A, rpc)
    sub = rpc if nwv == 1 else ((rpc // nwv) + 63) & ~63
    cbeg = np.arange(nchunks)[:, None] * rpc
    cend = np.minimum(A, cbeg + rpc)
    rbeg = cbeg + np.arange(nwv)[None, :] * sub
    rb = np.minimum(rbeg, A)
    rend = np.maximum(np.minimum(cend, rbeg + sub), rb)
    return cum[:, rend] - cum[:, rb], rbeg >= cend


def census():
    """-> {edge name: number of launches of the chosen cases that contain it}"""
    seen = {}

    def mark(name, yes):
        seen[name] = seen.get(name, 0) + int(bool(yes))

    for case in launched_cases():
        entry, K, rows, cin, cout, v, one = case
        for g, kind, level, swap in launches_of(case):
            nbr = table_np(g, kind, level)
            pick, info = plan_of(case, nbr.shape[1])
            p = parts(pick)
            if p["family"] == PIPE:
                n, empty = wave_rule_counts(nbr, info[I_RPC], p["nwv"])
                assert n.shape[1] == info[I_CHUNKS]
                d4 = 4 * p["d"]
                mark("wgrad2 n = 0", (n == 0).any())
                mark("wgrad2 0 < n < 4", ((n > 0) & (n < 4)).any())
                mark("wgrad2 n % 4 != 0", (n % 4 != 0).any())
                mark("wgrad2 0 < n <= 4 D", ((n > 0) & (n <= d4)).any())
                mark("wgrad2 n > 4 D", (n > d4).any())
                mark("wgrad2 n > 1024", (n > WG2_CAP).any())
                mark("wgrad2 NWV = 4, waves 1..3 empty", p["nwv"] == 4 and empty[:, 1:].all(1).any())
                mark("wgrad2 more than one Cin block", info[I_BLOCKS] > K * info[I_CHUNKS])
                mark("wgrad2 more than one chunk", info[I_CHUNKS] > 1)
            elif p["family"] == RUN:
                S = info[I_S]
                counts = (nbr >= 0).sum(1)
                sizes = [min(S, int(c) - i * S) for c in counts for i in range(cdiv(int(c), S))]
                tiles = {cdiv(s, WGR_TS) for s in sizes}
                assert sum(cdiv(int(c), S) for c in counts) <= info[I_PIECES]
                mu_w = [min(p["mu"], max(cin // 16 - w * p["mu"], 0)) for w in range(4)]
                mark("run piece of fewer than 32 slots", any(s < WGR_TS for s in sizes))
                for t in (1, 2, 3):
                    mark(f"run piece of {t} tiles", t in tiles)
                mark("run odd tile count", any(t % 2 for t in tiles))
                mark("run even tile count", any(t % 2 == 0 for t in tiles))
                mark("run offset with no rule", (counts == 0).any())
                mark("run >= 3 pieces, last shorter", any(c > 2 * S and c % S for c in counts))
                mark("run 0 < mu_w < MU", any(0 < m < p["mu"] for m in mu_w))
                mark("run mu_w == 0", 0 in mu_w)
                mark("run swap = 1", swap)
                mark("run LDS above 64 KB", info[I_LDS] > 64 << 10)
    return seen


# ---- the device side
SENTINEL = -777.0
COL0 = 4
TAIL = 64   # sentinel floats behind the workspace and around dW


class WBench:
    """Geometries on the device (the four of tests/_spconv_cases.py, checked against the oracle's by tests/test_gpu_spconv_kernels.py,
    and `cube15`), and per (table, cin, cout) the inputs as slices of NaN buffers, the float64 reference and the table entry's own
    result -- each built once and left unchanged."""

    def __init__(self):
        import torch
        from mopa_amd.sparse3d import Geometry3D
        self.g, self._dev, self._runs, self._none = {}, {}, {}, {}
        for name in GEOMETRIES:
            coords, levels, fs = geometry_coords(name)
            self.g[name] = Geometry3D(torch.from_numpy(coords), levels, fs, "cuda")
            o = oracle_geometry(name)
            assert tuple(self.g[name].num_active) == tuple(o.num_active)
            for kind in ("nbr27", "ch", "up"):
                for a, b in zip(getattr(self.g[name], kind), getattr(o, kind)):
                    assert np.array_equal(a.cpu().numpy(), np.asarray(b)), (name, kind)

    def table(self, name, kind, level):
        return getattr(self.g[name], kind)[level]

    def build_runs(self, tab):
        import torch
        from mopa_amd._lib import call, query, stream
        K, A = tab.shape
        buf = torch.empty(query("mopa_rulebook_runs_bytes", K, A) // 4, dtype=torch.int32, device="cuda")
        desc = np.asarray([(tab.data_ptr(), K, A, buf.data_ptr())], dtype=np.int64)
        call("mopa_rulebook_runs_build_batched", desc.ctypes.data, 1, stream())
        return buf

    def runs(self, name, kind, level):
        key = (name, kind, level)
        if key not in self._runs:
            tab = self.table(name, kind, level)
            r = self.g[name].runs(tab)
            self._runs[key] = r[0] if r is not None else self.build_runs(tab)
        return self._runs[key]

    def no_rules(self, K, A):
        """A table whose every entry is -1, and its run lists"""
        import torch
        if (K, A) not in self._none:
            tab = torch.full((K, A), -1, dtype=torch.int32, device="cuda")
            self._none[(K, A)] = (tab, self.build_runs(tab))
        return self._none[(K, A)]

    def case(self, name, kind, level, cin, cout):
        """-> dict: x / g as numpy, reference, allowed error, scale, the operand buffers built from them so far (operand()), the
        table entry's own result"""
        import torch
        key = (name, kind, level, cin, cout)
        hit = self._dev.get(key)
        if hit is None:
            x, g, ref = reference(*key)
            hit = dict(ref=torch.tensor(ref.reshape(-1), device="cuda"), scale=max(1.0, float(np.abs(ref).max())), x=x, g=g, buf={})
            hit["allowed"] = ATOL * hit["scale"] + RTOL * hit["ref"].abs()
            self._dev[key] = hit
        return hit

    def operand(self, hit, which, ld, col):
        """The rows of x or g at stride ld from float `col` of a flat buffer of NaN: with ld > C and col > 0 (every layout but the
        plain one) a channel slice with NaN in the other columns, in front of the first row and behind the last"""
        import torch
        k = (which, ld, col)
        if k not in hit["buf"]:
            a = hit[which]
            buf = torch.full((a.shape[0] * ld + 16,), float("nan"), device="cuda")
            buf[col:col + a.shape[0] * ld].view(a.shape[0], ld)[:, :a.shape[1]] = torch.tensor(a, device="cuda")
            hit["buf"][k] = buf
        return hit["buf"][k]

    def launch(self, case, name, kind, level, swap, accumulate=0, prev=None, tab=None, runs=None, use_stated=True):
        """One launch of a case through the C ABI on a table of a geometry, the stated size in `accumulate`.
        -> (kernel name the query gives for this very call, flat dW buffer with TAIL sentinels on both sides of a window that is only
        4-byte aligned, workspace with TAIL sentinels behind the queried size)."""
        import torch
        from mopa_amd._lib import call, ptr, stream
        entry, K, rows, cin, cout, v, one = case
        dli, dlo, li, lo, lw = (TABLE_VARIANTS, RUN_VARIANTS)[entry][v]
        assert (li | lo) % 4 == 0 and lw == 0
        t = self.table(name, kind, level) if tab is None else tab
        assert t.shape[0] == K
        A_out = t.shape[1]
        # swap = 1: the launch reads the deconvolution table's lists, x lives on its output (fine) rows and g on its input rows
        hit = self.case(name, "ch" if swap else kind, level, cin, cout)
        ld_in, ld_do = cin + dli, cout + dlo
        # slices: column COL0 of a row keeps 16-byte alignment when ld % 4 == 0; li / lo move the base by whole floats
        xcol, gcol = (COL0 if dli >= 8 else 0) + li // 4, (COL0 if dlo >= 8 else 0) + lo // 4
        xb, gb = self.operand(hit, "x", ld_in, xcol), self.operand(hit, "g", ld_do, gcol)
        assert (ptr(xb, xcol) & 15) == li and (ptr(gb, gcol) & 15) == lo
        acc = (stated(rows) if use_stated else 0) | accumulate
        pick, info = ask(entry, K, A_out, cin, cout, v, one, acc)
        assert pick > 0, (case, pick)
        n = K * cin * cout
        flat = torch.full((n + 2 * TAIL + 1,), SENTINEL, device="cuda")
        dw = flat[TAIL + 1:TAIL + 1 + n]
        if prev is not None:
            dw.copy_(prev)
        nws = info[I_WS] // 4
        ws = torch.full((nws + TAIL,), SENTINEL, device="cuda")
        assert ptr(ws) % 16 == 0
        if entry == 0:
            call("mopa_spconv_bwd_weight", ptr(t), K, A_out, ptr(xb, xcol), ld_in, cin, ptr(gb, gcol), ld_do, cout, ptr(dw), acc, ptr(ws), 4 * nws,
                 stream())
        else:
            r = self.runs(name, kind, level) if runs is None else runs
            call("mopa_spconv_bwd_weight_run", ptr(r), K, A_out, one, swap, ptr(xb, xcol), ld_in, cin, ptr(gb, gcol), ld_do, cout, ptr(dw), acc,
                 ptr(ws), 4 * nws, stream())
        return kernel_name(pick), flat, ws, nws

    def own_choice(self, name, kind, level, cin, cout):
        """The table entry's result with nothing stated and plain operands: what the other launches' bits are compared with."""
        hit = self.case(name, kind, level, cin, cout)
        if "own" not in hit:
            K = self.table(name, kind, level).shape[0]
            _, flat, _, _ = self.launch((0, K, 0, cin, cout, 0, 0), name, kind, level, 0)
            hit["own"] = flat[TAIL + 1:TAIL + 1 + K * cin * cout].clone()
        return hit["own"]

    def measure(self, case, name, kind, level, swap):
        """Three launches of a case on one table.  -> (kernel name, device vector [worst error / allowed error, worst error /
        max(1, max|ref|), every sentinel untouched, the second launch's bits equal the first's, worst |(prev + result) - accumulated|
        over its bound, the bits equal the table entry's own choice])."""
        import torch
        entry, K, rows, cin, cout, v, one = case
        hit = self.case(name, "ch" if swap else kind, level, cin, cout)
        own = self.own_choice(name, "ch" if swap else kind, level, cin, cout)
        n = K * cin * cout
        kname, flat, ws, nws = self.launch(case, name, kind, level, swap)
        got = flat[TAIL + 1:TAIL + 1 + n]
        err = (got.double() - hit["ref"]).abs()
        ratio = torch.nan_to_num(err / hit["allowed"], nan=float("inf")).max()
        quiet = (flat[:TAIL + 1] == SENTINEL).all() & (flat[TAIL + 1 + n:] == SENTINEL).all() & (ws[nws:] == SENTINEL).all()
        _, flat2, ws2, _ = self.launch(case, name, kind, level, swap)
        prev = torch.from_numpy(np.random.Generator(np.random.PCG64(n)).standard_normal(n, dtype=np.float32)).cuda()
        _, flat3, ws3, _ = self.launch(case, name, kind, level, swap, accumulate=1, prev=prev)
        quiet = quiet & (flat3[:TAIL + 1] == SENTINEL).all() & (flat3[TAIL + 1 + n:] == SENTINEL).all() & (ws3[nws:] == SENTINEL).all()
        acc_bound = 2e-6 * hit["scale"] + 1e-6 * prev.abs().max()   # (tests/test_gpu_3d.py, the run-list gradient's accumulation)
        acc = torch.nan_to_num(((flat3[TAIL + 1:TAIL + 1 + n] - prev) - got).abs().max() / acc_bound, nan=float("inf"))
        return kname, torch.stack([ratio, torch.nan_to_num(err, nan=float("inf")).max() / hit["scale"], quiet.double(),
                                   (flat == flat2).all().double(), acc.double(), (got == own).all().double()])
