"""Which kernel a sparse-convolution weight-gradient launch runs (mopa_spconv_wgrad_kernel; csrc/spconv.hip pick_wgrad,
csrc/sprun.hip wgr_pick) -- pure host queries, no GPU:

  * over K = 8 and 27, every (cin, cout) in multiples of 16 up to 256 x 112, the network's pairs, ragged pairs that reach all 28
    forms of the simple kernel and three wider ones, rows just under, at and over every threshold of the rules, eight operand
    layouts per entry point, the query -- kernel, chunks, rows per chunk, piece size and count, workspace and LDS bytes, blocks --
    equals a restatement of the dispatch as it stood before there was one decision per launch (wgrad_plan, stem_wgrad_shape, the
    `aligned` expression and `four` of mopa_spconv_bwd_weight / launch_wgrad, wgr_plan of mopa_spconv_bwd_weight_run, transcribed
    below), refusals included;
  * the witness table (tests/_spconv_wgrad_cases.py) holds one case per instantiation the enumeration reaches, stating a table size
    in bits 8-30 of `accumulate` selects for a 393-row table exactly what the rules select for a table of the stated size, and a
    stated size never lets a launch need more workspace than the query reports;
  * 22 of the 28 one-wave forms of k_spconv_wgrad2 are not reached with K = 8 or 27 and cin <= 256 (asserted, with the reason);
  * the weight-gradient launches of the 7-level, m = 16 network at the levels of 8 scans are pinned by name;
  * the cases the GPU test launches contain every kernel edge listed in census();
  * on the float64 reference alone: four single defects of the kind these kernels could have move the result by more than ten times
    the bound the GPU test (tests/test_gpu_spconv_wgrad_kernels.py) allows, on every launched table of at least 64 rows (the
    exchange of two accumulator rows has no meaning for the stem's single input channel and is not applied to it)."""
import math

import numpy as np
import pytest

import _spconv_wgrad_cases as W
from test_spconv_plan import KINDS, ROWS_8_SCANS, programs, q

cdiv = W.cdiv


def align256(n):
    return cdiv(n, 256) * 256


# ---- the dispatch as the two entry points spelled it out before pick_wgrad / wgr_pick
def old_plan(K, A, cin, cout):
    mt = cdiv(cin, 16)
    mu = next(c for c in (4, 3, 2, 1) if mt % c == 0)
    mb = mt // mu
    pipelined = cin % 16 == 0 and cout % 16 == 0
    waves = 16384 if not pipelined else 512 if K != 27 else 4096 if cout <= 16 else 512 if A < 4096 else 2048
    nc = max(1, min(cdiv(waves, K * mb), cdiv(A, 256), (32 << 20) // (K * cin * cout * 4) + 1, 2048))
    rpc = cdiv(cdiv(A, nc), 64) * 64
    return mu, mb, cdiv(A, rpc), rpc


def old_table(K, A, cin, cout, ld_in, ld_dout, in_low, dout_low):
    """-> (kernel, chunks, rows per chunk, S, pieces, workspace bytes, LDS bytes, blocks), or None where the call returns MOPA_ERR_ARG"""
    if K <= 0 or A <= 0 or cin <= 0 or cout <= 0 or cout > 112 or ld_in < cin or ld_dout < cout:
        return None
    mu, mb, nc, rpc = old_plan(K, A, cin, cout)
    ws = align256(nc * K * cin * cout * 4)
    if K <= 27 and cin == 1 and cout == 16:   # stem_wgrad_shape
        nb = min(cdiv(A, 256), 512)
        rpb = cdiv(cdiv(A, nb), 64) * 64
        nb = cdiv(A, rpb)
        ws = max(ws, align256(nb * K * 16 * 4))
        if ld_dout % 4 == 0 and dout_low == 0:
            return "k_spconv_stem_wgrad<16>", nb, rpb, 0, 0, ws, 0, nb
    nt = cdiv(cout, 16)
    aligned = (cin % 16 == 0 and cout % 16 == 0 and A * ld_dout < 1 << 32 and A * 8 * ld_in < 1 << 32 and (in_low | dout_low) & 3 == 0)
    grid = K * nc * mb
    if not aligned:
        return f"k_spconv_wgrad<{mu},{nt}>", nc, rpc, 0, 0, ws, 0, grid
    d = 8 if mu + nt <= 6 else 8 if mu <= 2 else 6
    nwv = 4 if grid <= 4200 and mu * nt <= 16 else 1
    return f"k_spconv_wgrad2<{mu},{nt},{d},{nwv}>", nc, rpc, 0, 0, ws, nwv * 2 * (1024 + 64) * 4 + mu * nt * 4 * 64 * 4, grid


def old_stride(c, n16):
    s = (c + 3) & ~3
    while s & 63 != (16 * n16) & 63:
        s += 4
    return s


def old_run(K, A, cin, cout, one, ld_in, ld_dout, ptr_low):
    if A <= 0 or not 0 < K <= 27 or not 16 <= cin <= 256 or cin % 16 or not 16 <= cout <= 112 or cout % 16:
        return None
    if ld_in < cin or ld_dout < cout or ld_in & 3 or ld_dout & 3 or ptr_low:
        return None
    mu, nt = (cin // 16 + 3) // 4, cout // 16
    lds = max(2 * 32 * (old_stride(cin, mu) + old_stride(cout, nt)) * 4 + 512 * 16, 4 * mu * nt * 4 * 64 * 4)
    S = min(max(W.raw_piece(K, one, A), 128), 1024)
    bound = A + K * 128 if one else cdiv(K * A + K * 128, 128) * 128
    while (bound // S + K) * cin * cout * 4 > 128 << 20:
        S += 32
    pieces = bound // S + K
    return f"k_wgrad_run<{mu},{nt}>", 0, 0, S, pieces, align256(pieces * cin * cout * 4), lds, pieces


def old_launch(case):
    entry, K, rows, cin, cout, v, one = case
    dli, dlo, li, lo, lw = (W.TABLE_VARIANTS, W.RUN_VARIANTS)[entry][v]
    if entry == 0:
        return old_table(K, rows, cin, cout, cin + dli, cout + dlo, li, lo)
    return old_run(K, rows, cin, cout, one, cin + dli, cout + dlo, li | lo | lw)


@pytest.fixture(scope="module")
def picks():
    return W.enumerate_picks()


def test_the_query_equals_the_dispatch_as_it_was_spelled_out(picks):
    assert len(picks) > 300000
    refused = 0
    for case, (pick, info) in picks.items():
        want = old_launch(case)
        if want is None:
            assert pick == -1 and not any(info), (case, pick, info)
            refused += 1
        else:
            assert pick > 0 and (W.kernel_name(pick),) + info == want, (case, hex(pick), info, want)
    assert refused > 100000 and len(picks) - refused > 300000   # (the run entry refuses every ragged or wide pair and six of its eight layouts)
    assert {c[5] for c, (p, _) in picks.items() if c[0] == 1 and c[3:5] == (64, 32) and p < 0 and old_run(c[1], c[2], c[3], c[4], c[6], c[3], c[4], 0)} == {2, 3, 4, 5, 6, 7}
    # rows x ld past 2^32: the pipelined kernel's 32-bit row offsets give way to the simple kernel, for either operand
    for cin, cout in ((64, 32), (256, 16)):
        for ld, v in ((8 * cin, 0), (8 * (cin + 3), 1)):   # (8 ld_in >= 128 > ld_dout: the input's test is the one that binds)
            r = cdiv(1 << 32, ld)
            assert W.kernel_name(picks[(0, 27, r - 1, cin, cout, v, 0)][0]).startswith("k_spconv_wgrad2<")
            assert W.kernel_name(picks[(0, 27, r, cin, cout, v, 0)][0]).startswith("k_spconv_wgrad<")


ONE_WAVE_FORMS_REACHED = {"k_spconv_wgrad2<1,1,8,1>", "k_spconv_wgrad2<3,6,6,1>", "k_spconv_wgrad2<3,7,6,1>", "k_spconv_wgrad2<4,5,6,1>",
                          "k_spconv_wgrad2<4,6,6,1>", "k_spconv_wgrad2<4,7,6,1>"}


def test_witness_table_reaches_every_instantiation_through_the_stated_size(picks):
    table = W.witness_table()
    reached = {W.witness_key(c, p) for c, (p, _) in picks.items() if p > 0}
    assert set(table) == reached
    names = {k[3] for k in table}
    mu_nt = [(m, n) for m in range(1, 5) for n in range(1, 8)]
    assert {f"k_spconv_wgrad<{m},{n}>" for m, n in mu_nt} <= names and {f"k_wgrad_run<{m},{n}>" for m, n in mu_nt} <= names
    depth = lambda m, n: 8 if m + n <= 6 or m <= 2 else 6
    assert {f"k_spconv_wgrad2<{m},{n},{depth(m, n)},4>" for m, n in mu_nt if m * n <= 16} <= names and "k_spconv_stem_wgrad<16>" in names
    # The one-wave form of k_spconv_wgrad2 needs a grid of more than 4,200 blocks or MU x NT > 16.  The wave target of the pipelined
    # kernel is at most 4,096 (27 offsets, cout = 16) -- the grid K x chunks x mblocks exceeds it by less than one K x mblocks -- and
    # 2,048 or 512 elsewhere, so below MU x NT = 17 only 208 -> 16 (13 blocks of Cin: 12 x 351 = 4,212 blocks) gets there: 22 of the
    # 28 compiled one-wave forms are never launched with 8 or 27 offsets and up to 256 input channels, the range enumerated here
    # (the entry point does not cap cin: 27 offsets, 368 -> 16 or 416 -> 16 also give 12 x 351 blocks, <1,1,8,1> and <2,1,8,1>).  (They were the long levels' form while the wave target
    # was 16,384; the kernels stay in place.)
    assert {n for n in names if n.startswith("k_spconv_wgrad2<") and n.endswith(",1>")} == ONE_WAVE_FORMS_REACHED
    assert W.kernel_name(W.ask(0, 27, 64 * 4100, 416, 16)[0]) == "k_spconv_wgrad2<2,1,8,1>" and W.kernel_name(W.ask(0, 27, 64 * 4100, 368, 16)[0]) == "k_spconv_wgrad2<1,1,8,1>"
    assert len(names) == 28 + 23 + 6 + 1 + 28
    for (entry, K, one, name), case in table.items():
        _, _, rows, cin, cout, v, _ = case
        small, info = W.ask(entry, K, 393, cin, cout, v, one, W.stated(rows))
        assert W.kernel_name(small) == name and small == picks[case][0], (case, name)
        # and the default is the table's own size: no bit above bit 0 set
        assert W.ask(entry, K, rows, cin, cout, v, one, 1) == picks[case], case
        # the layout the GPU test launches it in -- channel slices of buffers eight floats wider -- selects the same kernel and plan
        assert v == 0 and W.ask(entry, K, 393, cin, cout, W.sliced(case)[5], one, W.stated(rows)) == (small, info), case


def test_a_stated_size_never_outgrows_the_queried_workspace():
    """The slabs a launch writes are chunks x K x cin x cout (table entry; the stem: blocks x K x 16) or pieces x cin x cout floats
    (run entry: the grid is the piece count): whatever size is stated, the workspace the query reports covers them, and the chunk and
    piece counts stay within what the real table allows (256 rows per chunk, the bound on the slots)."""
    sizes = [0, 64, 640, 4096, 64 * 1000, 64 * 4100, 64 * 20000, 64 * ((1 << 23) - 1)]
    for case in W.launched_cases():
        entry, K, _, cin, cout, v, one = case
        for A in (1, 143, 393, 786, 3375):
            base = W.ask(entry, K, A, cin, cout, v, one, 0)
            for s in sizes:
                pick, info = W.ask(entry, K, A, cin, cout, v, one, W.stated(s) | 1)
                assert pick > 0
                if entry == 0:
                    assert info[W.I_CHUNKS] * K * cin * cout * 4 <= info[W.I_WS] and info[W.I_CHUNKS] <= cdiv(A, 256)
                    assert info[W.I_CHUNKS] * info[W.I_RPC] >= A and info[W.I_RPC] % 64 == 0
                else:
                    bound = A + K * 128 if one else cdiv(K * A + K * 128, 128) * 128   # slots that can hold a rule: sum_o ceil(n_o / S) <= bound / S + K
                    assert info[W.I_PIECES] == bound // info[W.I_S] + K == info[W.I_BLOCKS] and 128 <= info[W.I_S] <= 1024
                    assert info[W.I_PIECES] * cin * cout * 4 <= info[W.I_WS]
                if s == 0:
                    assert (pick, info) == base


# The weight-gradient launches of the 7-level, m = 16 network (plain and residual blocks hold the same convolution shapes) at the
# levels of 8 scans, read off csrc/spconv.hip and csrc/sprun.hip as they stood before the decision functions: (kind, level, cin,
# cout) -> kernel.  Entry point per launch: mopa_spconv_wgrad_plan (tests/test_spconv_plan.py).
PINNED = {
    ('subm', 0, 1, 16): 'k_spconv_stem_wgrad<16>',
    ('subm', 0, 16, 16): 'k_spconv_wgrad2<1,1,8,4>',
    ('down', 0, 16, 32): 'k_spconv_wgrad2<1,2,8,4>',
    ('subm', 1, 32, 32): 'k_spconv_wgrad2<2,2,8,4>',
    ('down', 1, 32, 48): 'k_wgrad_run<1,3>',
    ('subm', 2, 48, 48): 'k_wgrad_run<1,3>',
    ('down', 2, 48, 64): 'k_wgrad_run<1,4>',
    ('subm', 3, 64, 64): 'k_wgrad_run<1,4>',
    ('down', 3, 64, 80): 'k_wgrad_run<1,5>',
    ('subm', 4, 80, 80): 'k_spconv_wgrad2<1,5,8,4>',
    ('down', 4, 80, 96): 'k_spconv_wgrad2<1,6,8,4>',
    ('subm', 5, 96, 96): 'k_wgrad_run<2,6>',
    ('down', 5, 96, 112): 'k_spconv_wgrad2<3,7,6,1>',
    ('subm', 6, 112, 112): 'k_wgrad_run<2,7>',
    ('up', 5, 112, 96): 'k_spconv_wgrad2<1,6,8,4>',
    ('subm', 5, 192, 96): 'k_wgrad_run<3,6>',
    ('up', 4, 96, 80): 'k_spconv_wgrad2<3,5,6,4>',
    ('subm', 4, 160, 80): 'k_wgrad_run<3,5>',
    ('up', 3, 80, 64): 'k_wgrad_run<2,4>',
    ('subm', 3, 128, 64): 'k_wgrad_run<2,4>',
    ('up', 2, 64, 48): 'k_wgrad_run<1,3>',
    ('subm', 2, 96, 48): 'k_wgrad_run<2,3>',
    ('up', 1, 48, 32): 'k_wgrad_run<1,2>',
    ('subm', 1, 64, 32): 'k_wgrad_run<1,2>',
    ('up', 0, 32, 16): 'k_spconv_wgrad2<2,1,8,4>',
    ('subm', 0, 32, 16): 'k_spconv_wgrad2<2,1,8,4>',
    ('nin', 5, 192, 96): 'k_spconv_wgrad2<4,6,6,1>',
    ('nin', 4, 160, 80): 'k_spconv_wgrad2<2,5,8,4>',
    ('nin', 3, 128, 64): 'k_spconv_wgrad2<4,4,6,4>',
    ('nin', 2, 96, 48): 'k_spconv_wgrad2<3,3,8,4>',
    ('nin', 1, 64, 32): 'k_spconv_wgrad2<4,2,8,4>',
    ('nin', 0, 32, 16): 'k_spconv_wgrad2<2,1,8,4>',
}


def network_launches(name_of):
    out = {}
    rows = ROWS_8_SCANS
    for prog in programs():
        for op in prog.ops:
            if op[0] != "conv":
                continue
            _, _, kind, l, src, dst = op
            if kind == "subm":
                tab, rev = (27, rows[l], 0), (27, rows[l], 0)
            elif kind == "nin":
                tab, rev = (1, rows[l], 0), (1, rows[l], 0)
            elif kind == "down":
                tab, rev = (8, rows[l + 1], 0), (8, rows[l], 1)
            else:
                tab, rev = (8, rows[l], 1), (8, rows[l + 1], 0)
            has = [q("mopa_rulebook_runs_wanted", *t) for t in (tab, rev)]
            plan = q("mopa_spconv_wgrad_plan", KINDS.index(kind), tab[0], tab[1], has[0], tab[2], rev[1], has[1], rev[2], src.C, dst.C)
            K, n, one = rev if plan == 2 else tab
            out[(kind, l, src.C, dst.C)] = name_of(int(plan != 0), K, n, src.C, dst.C, one)
    return out


def test_network_launches_at_8_scans_are_the_pinned_kernels():
    got = network_launches(lambda e, K, n, cin, cout, one: W.kernel_name(W.ask(e, K, n, cin, cout, 0, one)[0]))
    assert got == PINNED, {k: (got.get(k), PINNED.get(k)) for k in set(got) | set(PINNED) if got.get(k) != PINNED.get(k)}
    assert got == network_launches(lambda e, K, n, cin, cout, one: old_launch((e, K, n, cin, cout, 0, one))[0])


def test_the_launched_cases_contain_every_kernel_edge():
    seen = W.census()
    print({k: v for k, v in sorted(seen.items())})
    assert len(seen) == 9 + 12 and all(v > 0 for v in seen.values()), sorted(k for k, v in seen.items() if not v)
    # the list of more than 1,024 rules is the one the issue names: 27 offsets, three chunks of 1,152 rows, one wave per chunk
    pick, info = W.plan_of((0, 27, 0, 336, 96, 0, 0), 3375)
    assert W.kernel_name(pick) == "k_spconv_wgrad2<3,6,6,1>" and info[:2] == (3, 1152)


# ---- single defects on the float64 reference
def defects(case, name, kind, level, swap):
    """-> {defect: worst |defective - reference| / allowed error} for one launch of a case: the four defects applied where the launch's
    own plan puts them (its chunks or pieces, its lists), on the densest offset of the table."""
    entry, K, rows, cin, cout, v, one = case
    tkind = "ch" if swap else kind
    nbr = W.table_np(name, tkind, level)
    x, g, ref = W.reference(name, tkind, level, cin, cout)
    ok = W.allowed(ref)
    counts = (nbr >= 0).sum(1)
    o = int(np.argmax(counts))
    out_rows = np.flatnonzero(nbr[o] >= 0)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)

    def part(rws):   # the contribution of some rules of offset o
        return x64[nbr[o, rws]].T @ g64[rws]

    worst = lambda delta: float((np.abs(delta) / ok[o]).max())
    pick, info = W.plan_of(case, W.table_np(name, kind, level).shape[1])
    if entry == 0:   # the chunk (or stem block) that holds the offset's last rule; the list of its last wave
        rpc = info[W.I_RPC]
        c0 = out_rows[-1] // rpc * rpc
        slab = out_rows[out_rows >= c0]
        nwv = max(W.parts(pick)["nwv"], 1)
        sub = rpc if nwv == 1 else ((rpc // nwv) + 63) & ~63
        lst = slab[slab >= c0 + (out_rows[-1] - c0) // sub * sub]
    else:            # the offset's last piece of S rules in run order (ascending rows); its list is the piece
        S = info[W.I_S]
        slab = lst = out_rows[(len(out_rows) - 1) // S * S:]
    step = lst[len(lst) - ((len(lst) - 1) % 4 + 1):]
    a, b = 16 * ((cin - 1) // 16) + 1, 16 * ((cin - 1) // 16)   # two accumulator rows of the last 16-channel block (one row: cin = 1)
    exch = ref[o].copy()
    if cin > 1:
        exch[[a, b]] = exch[[b, a]]
    loud = out_rows[np.argmax(np.abs(x64[nbr[o, out_rows]]).max(1) * np.abs(g64[out_rows]).max(1))]   # (the stem has ONE input channel: a rule whose input is not near zero)
    return {"one rule dropped": worst(part(np.asarray([loud]))), "one slab left out": worst(part(slab)),
            "two accumulator rows exchanged": worst(exch - ref[o]) if cin > 1 else None, "last k-step of a list dropped": worst(part(step))}


def test_single_defects_exceed_ten_times_the_gpu_bound():
    n, lowest = 0, {}
    for case in W.launched_cases():
        for name, kind, level, swap in W.launches_of(case):
            if W.table_np(name, "ch" if swap else kind, level).shape[1] < 64:
                continue
            for defect, ratio in defects(case, name, kind, level, swap).items():
                if ratio is not None:
                    assert ratio > 10, (defect, ratio, case, name, kind, level, swap)
                    lowest[defect] = min(lowest.get(defect, math.inf), ratio)
                    n += 1
    print(n, "defects;", {k: round(v) for k, v in lowest.items()})
    assert n > 2000 and len(lowest) == 4
