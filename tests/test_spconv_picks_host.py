"""Which kernel a sparse-convolution forward launch runs (mopa_spconv_fwd_kernel; csrc/spconv.hip pick_fwd / pick_grouped,
csrc/sprun_pack.h spk_pick_run) -- pure host queries, no GPU:

  * over K = 8 and 27, every channel pair in multiples of 16 up to 224, the network's pairs and the unaligned ones, rows just under,
    at and over every threshold of the rules, both weight forms, with and without a workspace, the query equals a restatement of
    the dispatch as it stood before there was one decision per launch (the nested ifs of mopa_spconv_fwd, mopa_spconv_fwd_grouped and
    mopa_spconv_fwd_run, transcribed below);
  * the witness table (tests/_spconv_cases.py) holds one case per instantiation the enumeration reaches, and stating a table size in
    bits 8-30 of w_flip selects for a 393-row table exactly what the rules select for a table of the stated size;
  * the launches of the 7-level, m = 16 network at the levels of 8 scans are pinned by name;
  * on the float64 reference alone: three single defects of the kind these kernels could have move the result by more than ten times
    the bound the GPU test (tests/test_gpu_spconv_kernels.py) allows."""
import numpy as np
import pytest

import _spconv_cases as C
from test_spconv_plan import ROWS_8_SCANS, programs, q


# ---- the dispatch as the three entry points spelled it out before pick_fwd / pick_grouped / spk_pick_run
def cdiv(a, b):
    return -(-a // b)


def old_fwd(K, rows, cin, cout, aligned):
    if cin <= 4 and cout in (16, 32):   # the stem: scalar gathers
        return f"k_spconv_stem<{cin},{cout}>"
    NT, tiles, ntw = cdiv(cout, 16), cdiv(rows, 64), 1
    for c in (4, 3, 2, 1):   # fwd_plan
        if NT % c == 0 and (tiles >= 1500 or tiles * (NT // c) >= 1024):
            ntw = c
            break
    if not aligned:
        ntw = 1
    c16 = cdiv(cin, 16)       # dispatch_fwd
    na = c16 if c16 <= 4 else 8 if cin <= 128 else 12
    return f"k_spconv_fwd<{ntw},{na},{'true' if aligned else 'false'}>"


def old_packed_plan(K, rows, cin, cout):
    """-> ('blk' | 'pipe' | 't4', ntw) with MOPA_SPCONV_PATH unset"""
    if cin % 16 or cout % 16 or cin > 224 or cout > 224:
        return "blk", 0
    tiles, nt = cdiv(rows, 64), cout // 16
    if cout == 16 and tiles >= 1500:
        return "pipe", 1
    w = 2 if nt % 2 == 0 else 3 if nt % 3 == 0 else 1
    if tiles * (nt // w) < 768:
        w = 1
    if tiles * (nt // w) >= 256:
        return "t4", w
    return "blk", 0


def old_blk_lds(ntw, cin):
    return (2 * (cdiv(cin, 16) * 16) * ntw * 16 + 4 * 64 * (ntw * 16 + 4)) * 4


def old_grouped(K, rows, cin, cout, packed, aligned, has_ws):
    """-> kernel name, or None where the call returns MOPA_ERR_ARG"""
    if cin > (224 if packed else 192):
        return None
    if packed:
        path, pntw = old_packed_plan(K, rows, cin, cout)
        if not aligned or path == "blk":
            return None
        nkc = cin // 16

        def t4(n, ku, d, wv=4):
            return f"k_spconv_t4<{n},{ku},{d},{'true' if nkc % ku else 'false'},{wv}>"
        if path == "pipe" and cout == 16 and nkc == 2:   # 32 -> 16: one wave per tile with whole-Cin units
            return t4(1, 2, 2, 1)
        if path == "pipe":
            return {1: "k_spconv_pipe<1,2,40>", 2: "k_spconv_pipe<2,6,32>", 3: "k_spconv_pipe<3,6,40>"}.get(cout // 16, "k_spconv_pipe<4,4,28>")
        if K != 27 and cdiv(rows, 64) > 800:   # long down/up tables
            if pntw in (1, 2):
                return t4(pntw, nkc if nkc <= 3 else 4, 2, 1)
            return t4(3, nkc if nkc <= 2 else 3, 2, 1)
        if pntw == 1:
            if nkc == 1:
                return t4(1, 1, 4)
            if nkc == 2:
                return t4(1, 2, 2)
            for ku in (5, 7, 3):
                if nkc % ku == 0:
                    return t4(1, ku, 2)
            return t4(1, 4, 2)
        if pntw == 2:
            if nkc in (1, 2):
                return t4(2, nkc, 2)
            for ku in (5, 3):
                if nkc % ku == 0:
                    return t4(2, ku, 2)
            return t4(2, 4, 2)
        if nkc == 1:
            return t4(3, 1, 2)
        if nkc in (2, 4):
            return t4(3, 2, 2)
        return t4(3, 3, 2)
    NT, ntw = cdiv(cout, 16), 1
    if aligned:   # blk_plan
        tiles4 = cdiv(cdiv(rows, 64), 4)
        for c in (4, 2, 1):
            if NT % c or old_blk_lds(c, cin) > 64 * 1024:
                continue
            ntw = c
            if tiles4 * (NT // c) >= 512:
                break
    if old_blk_lds(ntw, cin) > 64 * 1024:
        return None
    osplit = 1
    if aligned and has_ws:   # blk_osplit
        blocks = cdiv(cdiv(rows, 64), 4) * cdiv(NT, ntw)
        osplit = max(1, min(cdiv(3072, blocks), 9, (48 << 20) // (rows * cout * 4 + 1), K // 2))
    c16 = cdiv(cin, 16)       # dispatch_blk_c
    na = c16 if c16 <= 4 else 8 if c16 <= 8 else 12
    return f"k_spconv_blk<{ntw},{na},{'true' if aligned else 'false'}>" + (f" osplit {osplit}" if osplit > 1 else "")


def old_run(K, rows, cin, cout, one):
    if cin % 16 or cout % 16 or not 16 <= cin <= 224 or not 16 <= cout <= 224:   # run_nt
        return None
    tiles = cout // 16
    nt = tiles if tiles <= 7 else next((c for c in range(7, 1, -1) if tiles % c == 0), 0)
    if nt == 0:
        return None
    rules_est = 9 * rows if K == 27 else rows if one else 5 * rows // 2
    return f"k_spconv_run<{nt},{1 if rules_est // 128 < 1024 else 2},{'true' if one else 'false'}>"


def old_kernel(case):
    entry, K, rows, cin, cout, packed, has_ws, one = case
    aligned = cin % 16 == 0 and cout % 16 == 0
    if entry == 0:
        return old_fwd(K, rows, cin, cout, aligned) if cin <= 192 else None
    if entry == 1:
        return old_grouped(K, rows, cin, cout, packed, aligned, has_ws)
    return old_run(K, rows, cin, cout, one)


@pytest.fixture(scope="module")
def picks():
    return C.enumerate_picks()


def test_the_query_equals_the_dispatch_as_it_was_spelled_out(picks):
    assert len(picks) > 400000
    refused = 0
    for case, pick in picks.items():
        want = old_kernel(case)
        if want is None:
            assert pick < 0, (case, hex(pick))
            refused += 1
        else:
            assert pick > 0 and C.kernel_name(pick) == want, (case, hex(pick), want)
    assert 0 < refused < len(picks) // 2


def test_witness_table_reaches_every_instantiation_through_the_stated_size(picks):
    table = C.witness_table()
    reached = {(c[0], c[1], C.kernel_name(p)) for c, p in picks.items() if p > 0}
    assert set(table) == reached
    names = {k[2] for k in table}
    # what the kernel-level tests at 5,000 to 20,000 rows never launch
    for must in ("k_spconv_t4<2,2,2,false,4>", "k_spconv_t4<3,3,2,true,4>", "k_spconv_t4<1,4,2,true,1>", "k_spconv_t4<3,3,2,false,1>",
                 "k_spconv_pipe<1,2,40>", "k_spconv_fwd<4,8,true>", "k_spconv_fwd<3,12,true>", "k_spconv_blk<2,4,true>", "k_spconv_blk<2,8,true>", "k_spconv_blk<1,12,true>",
                 "k_spconv_blk<1,8,true> osplit 9", "k_spconv_run<7,2,false>", "k_spconv_run<1,2,true>", "k_spconv_fwd<1,2,false>",
                 "k_spconv_blk<1,2,false>", "k_spconv_stem<4,16>"):
        assert must in names, must
    assert not any(n.startswith(("k_spconv_pipe<2", "k_spconv_pipe<3", "k_spconv_pipe<4")) for n in names)   # MOPA_SPCONV_PATH=1 only
    # 64-column blocks never fit: four waves' accumulators alone are 4 x 64 x 68 x 4 bytes > 64 KB (blk_lds_bytes), so blk_plan skips them
    assert not any(n.startswith("k_spconv_blk<4") for n in names)
    for (entry, K, name), case in table.items():
        _, _, rows, cin, cout, packed, has_ws, one = case
        small = C.pick_of(entry, K, 393, cin, cout, w_flip=C.stated(rows) | 2 * packed, has_ws=has_ws, one=one)
        assert C.kernel_name(small) == name and small == picks[case], (case, name)
        # and the default is the table's own size: no bit above bit 1 set
        assert C.pick_of(entry, K, rows, cin, cout, w_flip=2 * packed | 1, has_ws=has_ws, one=one) == picks[case]


# The forward and backward-data launches of the 7-level, m = 16 network (plain and residual blocks hold the same convolution shapes) at
# the levels of 8 scans, read off csrc/spconv.hip and csrc/sprun.hip as they stood before the decision functions: (kind, level, cin,
# cout, backward-data) -> kernel.  Path per launch: mopa_spconv_plan (tests/test_spconv_plan.py).
PINNED = {
    ('subm', 0, 1, 16, 0): 'k_spconv_stem<1,16>',
    ('subm', 0, 16, 16, 0): 'k_spconv_pipe<1,2,40>',
    ('subm', 0, 32, 16, 0): 'k_spconv_t4<1,2,2,false,1>',
    ('subm', 0, 16, 1, 1): 'k_spconv_fwd<1,1,false>',
    ('subm', 0, 16, 16, 1): 'k_spconv_pipe<1,2,40>',
    ('subm', 0, 16, 32, 1): 'k_spconv_t4<2,1,2,false,4>',
    ('nin', 0, 32, 16, 0): 'k_spconv_fwd<1,2,true>',
    ('nin', 0, 16, 32, 1): 'k_spconv_fwd<2,1,true>',
    ('down', 0, 16, 32, 0): 'k_spconv_t4<2,1,2,false,1>',
    ('down', 0, 32, 16, 1): 'k_spconv_run<1,2,true>',
    ('up', 0, 32, 16, 0): 'k_spconv_run<1,2,true>',
    ('up', 0, 16, 32, 1): 'k_spconv_t4<2,1,2,false,1>',
    ('subm', 1, 32, 32, 0): 'k_spconv_t4<2,2,2,false,4>',
    ('subm', 1, 64, 32, 0): 'k_spconv_t4<2,4,2,false,4>',
    ('subm', 1, 32, 32, 1): 'k_spconv_t4<2,2,2,false,4>',
    ('subm', 1, 32, 64, 1): 'k_spconv_t4<2,2,2,false,4>',
    ('nin', 1, 64, 32, 0): 'k_spconv_fwd<2,4,true>',
    ('nin', 1, 32, 64, 1): 'k_spconv_fwd<4,2,true>',
    ('down', 1, 32, 48, 0): 'k_spconv_t4<3,2,2,false,1>',
    ('down', 1, 48, 32, 1): 'k_spconv_run<2,2,true>',
    ('up', 1, 48, 32, 0): 'k_spconv_run<2,2,true>',
    ('up', 1, 32, 48, 1): 'k_spconv_t4<3,2,2,false,1>',
    ('subm', 2, 48, 48, 0): 'k_spconv_t4<3,3,2,false,4>',
    ('subm', 2, 96, 48, 0): 'k_spconv_run<3,2,false>',
    ('subm', 2, 48, 48, 1): 'k_spconv_t4<3,3,2,false,4>',
    ('subm', 2, 48, 96, 1): 'k_spconv_t4<2,3,2,false,4>',
    ('nin', 2, 96, 48, 0): 'k_spconv_fwd<3,8,true>',
    ('nin', 2, 48, 96, 1): 'k_spconv_fwd<3,3,true>',
    ('down', 2, 48, 64, 0): 'k_spconv_t4<2,3,2,false,4>',
    ('down', 2, 64, 48, 1): 'k_spconv_run<3,1,true>',
    ('up', 2, 64, 48, 0): 'k_spconv_run<3,1,true>',
    ('up', 2, 48, 64, 1): 'k_spconv_t4<2,3,2,false,4>',
    ('subm', 3, 64, 64, 0): 'k_spconv_run<4,2,false>',
    ('subm', 3, 128, 64, 0): 'k_spconv_run<4,2,false>',
    ('subm', 3, 64, 64, 1): 'k_spconv_run<4,2,false>',
    ('subm', 3, 64, 128, 1): 'k_spconv_run<4,2,false>',
    ('nin', 3, 128, 64, 0): 'k_spconv_fwd<2,8,true>',
    ('nin', 3, 64, 128, 1): 'k_spconv_fwd<4,4,true>',
    ('down', 3, 64, 80, 0): 'k_spconv_t4<1,4,2,false,4>',
    ('down', 3, 80, 64, 1): 'k_spconv_run<4,1,true>',
    ('up', 3, 80, 64, 0): 'k_spconv_run<4,1,true>',
    ('up', 3, 64, 80, 1): 'k_spconv_t4<1,4,2,false,4>',
    ('subm', 4, 80, 80, 0): 'k_spconv_run<5,2,false>',
    ('subm', 4, 160, 80, 0): 'k_spconv_run<5,2,false>',
    ('subm', 4, 80, 80, 1): 'k_spconv_run<5,2,false>',
    ('subm', 4, 80, 160, 1): 'k_spconv_run<5,2,false>',
    ('nin', 4, 160, 80, 0): 'k_spconv_fwd<1,12,true>',
    ('nin', 4, 80, 160, 1): 'k_spconv_fwd<2,8,true>',
    ('down', 4, 80, 96, 0): 'k_spconv_t4<1,5,2,false,4>',
    ('down', 4, 96, 80, 1): 'k_spconv_run<5,1,true>',
    ('up', 4, 96, 80, 0): 'k_spconv_run<5,1,true>',
    ('up', 4, 80, 96, 1): 'k_spconv_t4<1,5,2,false,4>',
    ('subm', 5, 96, 96, 0): 'k_spconv_run<6,1,false>',
    ('subm', 5, 192, 96, 0): 'k_spconv_run<6,1,false>',
    ('subm', 5, 96, 96, 1): 'k_spconv_run<6,1,false>',
    ('subm', 5, 96, 192, 1): 'k_spconv_run<6,1,false>',
    ('nin', 5, 192, 96, 0): 'k_spconv_fwd<1,12,true>',
    ('nin', 5, 96, 192, 1): 'k_spconv_fwd<1,8,true>',
    ('down', 5, 96, 112, 0): 'k_spconv_t4<1,3,2,false,4>',
    ('down', 5, 112, 96, 1): 'k_spconv_t4<1,7,2,false,4>',
    ('up', 5, 112, 96, 0): 'k_spconv_t4<1,7,2,false,4>',
    ('up', 5, 96, 112, 1): 'k_spconv_t4<1,3,2,false,4>',
    ('subm', 6, 112, 112, 0): 'k_spconv_run<7,1,false>',
    ('subm', 6, 112, 112, 1): 'k_spconv_run<7,1,false>',
}


def network_launches():
    """(kind, level, cin, cout, backward-data) -> kernel name the query gives, for every convolution of both programs"""
    out = {}
    rows = ROWS_8_SCANS
    for prog in programs():
        for op in prog.ops:
            if op[0] != "conv":
                continue
            _, _, kind, l, src, dst = op
            for rev in (False, True):
                if kind == "subm":
                    K, n, one = 27, rows[l], 0
                elif kind == "nin":
                    K, n, one = 1, rows[l], 0
                elif (kind == "down") != rev:
                    K, n, one = 8, rows[l + 1], 0
                else:
                    K, n, one = 8, rows[l], 1
                cin, cout = (dst.C, src.C) if rev else (src.C, dst.C)
                has_runs = q("mopa_rulebook_runs_wanted", K, n, one)
                plan = q("mopa_spconv_plan", K, n, cin, cout, cin, int(kind != "nin"), has_runs, one)
                path = plan >> 24
                pick = C.pick_of((0, 1, 1, 2)[path], K, n, cin, cout, w_flip=2 * (path == 2), has_ws=int(path in (1, 3)), one=one)
                out[(kind, l, cin, cout, int(rev))] = C.kernel_name(pick)
    return out


def test_network_launches_at_8_scans_are_the_pinned_kernels():
    got = network_launches()
    assert got == PINNED, {k: (got.get(k), PINNED.get(k)) for k in set(got) | set(PINNED) if got.get(k) != PINNED.get(k)}


# ---- single defects on the float64 reference
def conv64(x, nbr, w, drop_rule=None, swap_group=None, keep_groups=None):
    """out[i] = sum_o x[nbr[o, i]] @ w[o] in float64, offsets ascending, walked as the grouped kernels walk a table: per 64-row tile
    and offset the rules in groups of 16.  drop_rule = (o, i): that rule is skipped; swap_group = n: the n-th group of the table is
    multiplied with the next offset's weight; keep_groups = n: every tile stops after its first n groups."""
    K, A = nbr.shape
    out = np.zeros((A, w.shape[2]))
    g_all = 0
    for t in range(0, A, 64):
        g_tile = 0
        for o in range(K):
            rows = [i for i in range(t, min(t + 64, A)) if nbr[o, i] >= 0]
            for g0 in range(0, len(rows), 16):
                wo = w[(o + 1) % K] if swap_group == g_all else w[o]
                if keep_groups is None or g_tile < keep_groups:
                    for i in rows[g0:g0 + 16]:
                        if drop_rule != (o, i):
                            out[i] += x[nbr[o, i]] @ wo
                g_tile += 1
                g_all += 1
    return out


@pytest.mark.parametrize("cin,cout", [(16, 16), (48, 32)])
def test_single_defects_exceed_ten_times_the_gpu_bound(cin, cout):
    o = C.oracle_geometry("mixed")
    assert tuple(o.num_active) == C.EXPECT_ROWS["mixed"] and C.tile_groups(o.nbr27[0]) == C.EXPECT_GROUPS[("mixed", "nbr27", 0)]
    nbr = np.asarray(o.nbr27[0])
    x, w, ref = C.reference("mixed", "nbr27", 0, 0, cin, cout)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    clean = conv64(x64, nbr, w64)
    assert np.abs(clean - ref).max() < 1e-12   # the restatement is the oracle
    allowed = C.bound(ref) + C.RTOL * np.abs(ref)
    # the last rule of the table's last row (a 9-row tile of 3 groups), a group in the middle of the 96-group tile, and the groups
    # behind the first 48 of a tile (the second metadata chunk at MU = 48)
    last = max(oo for oo in range(27) if nbr[oo, -1] >= 0)
    for defect in (dict(drop_rule=(last, nbr.shape[1] - 1)), dict(swap_group=84 + 40), dict(keep_groups=48)):
        bad = conv64(x64, nbr, w64, **defect)
        assert (np.abs(bad - ref) / allowed).max() > 10, defect
