"""Every weight-gradient kernel of the sparse convolution (csrc/spconv.hip, csrc/sprun.hip) on tables of 1 to 3,375 rows against
dW[o] = X[in_rows(o)]^T G[out_rows(o)] in numpy float64 on the oracle's tables.  Run with -m gpu on an MI355X.

The dispatch picks an instantiation from the channel pair, the operands' layout and the table's row count; bits 8-30 of `accumulate`
state another row count for that choice alone, so the forms of the quarter-million-row levels run here on the geometries of
tests/_spconv_cases.py (their 27-offset, stride-2 and deconvolution tables) and on a 15^3 block whose chunks hold more than 1,024
rules (tests/_spconv_wgrad_cases.py; tests/test_spconv_wgrad_picks_host.py computes the witness table, counts the kernel edges
these launches contain and shows that single defects exceed the bound tenfold).  Per launch: the query names the witness's kernel;
the result is within rtol 2e-4 / atol 5e-5 max(1, max|ref|) (the weight-gradient bound of tests/test_gpu_3d.py); x and dout are
channel slices (ld = C + 8, column 4: 16-byte alignment kept) of buffers whose other columns are NaN -- every case on every table,
and on `mixed` also in the plain layout ld = C; dW is a 4-byte-aligned window of a flat buffer with sentinels on both sides; the
workspace has a sentinel tail behind the queried size; a second launch gives the same bits; accumulate = 1 onto a random previous value gives previous +
result within 2e-6 max(1, max|ref|) + 1e-6 max|previous| (the run-list test of tests/test_gpu_3d.py).  Whether a kernel's bits equal
those of the table entry's own choice is observed and printed, not asserted (chunking and piece order differ between forms)."""
import numpy as np
import pytest
import torch

import _spconv_wgrad_cases as W

pytestmark = pytest.mark.gpu

CHUNK = 20
GROUPS = [(0, 8, 0), (0, 27, 0), (1, 8, 0), (1, 8, 1), (1, 27, 0)]
LAUNCHED = {}   # witness key -> (launches, worst error / bound, worst error / max|ref|, launches with the table entry's own bits)


@pytest.fixture(scope="module")
def bench():
    return W.WBench()


def group_keys(group):
    return sorted(k for k in W.witness_table() if k[:3] == group)


CHUNKS = [(g, i) for g in GROUPS for i in range(3 if g[0] == 0 else 2)]


def run_case(bench, case, name=None, key=None):
    vecs = []
    for geom, kind, level, swap in W.launches_of(case):
        # on every table as channel slices of wider buffers of NaN; on `mixed` also in the plain layout (ld = C)
        for c in dict.fromkeys([W.sliced(case)] + ([case] if geom == "mixed" else [])):
            kname, v = bench.measure(c, geom, kind, level, swap)
            assert name is None or kname == name, (c, geom, kind, level, kname)   # the right kernel
            vecs.append(v)
    m = torch.stack(vecs).cpu().numpy()
    print(f"{W.ENTRIES[case[0]]} K {case[1]} {kname} {case[3]}->{case[4]}: {len(m)} launches, worst error {m[:, 0].max():.3f} of the bound, "
          f"{m[:, 1].max():.2e} of max|ref|, accumulate {m[:, 4].max():.3f} of its bound, the table entry's own bits in {int((m[:, 5] == 1).sum())}")
    assert (m[:, 0] <= 1).all(), (case, m[:, 0].max())          # accuracy
    assert (m[:, 2] == 1).all(), case                           # every sentinel untouched
    assert (m[:, 3] == 1).all(), case                           # determinism
    assert (m[:, 4] <= 1).all(), (case, m[:, 4].max())          # accumulate
    if key is not None:
        LAUNCHED[key] = (len(m), float(m[:, 0].max()), float(m[:, 1].max()), int((m[:, 5] == 1).sum()))
    return kname


def no_rules(bench, case):
    """A table whose every entry is -1: exact zeros, or the previous value bit for bit under accumulate."""
    entry, K, rows, cin, cout, v, one = case = W.sliced(case)
    tab, runs = bench.no_rules(K, 143)   # (the rows of `mixed` level 2: its inputs serve)
    n = K * cin * cout
    _, flat, _, _ = bench.launch(case, "mixed", "nbr27", 2, 0, tab=tab, runs=runs)
    prev = torch.from_numpy(np.random.Generator(np.random.PCG64(n)).standard_normal(n, dtype=np.float32)).cuda()
    _, flat2, _, _ = bench.launch(case, "mixed", "nbr27", 2, 0, accumulate=1, prev=prev, tab=tab, runs=runs)
    return (flat[W.TAIL + 1:W.TAIL + 1 + n] == 0).all() & (flat2[W.TAIL + 1:W.TAIL + 1 + n] == prev).all()


@pytest.mark.parametrize("group,i", CHUNKS)
def test_witnesses_vs_float64(bench, group, i):
    keys = group_keys(group)
    per = -(-len(keys) // (3 if group[0] == 0 else 2))
    zeros = []
    for key in keys[i * per:(i + 1) * per]:
        case = W.witness_table()[key]
        run_case(bench, case, key[3], key)
        zeros.append(no_rules(bench, case))
    assert bool(torch.stack(zeros).all())


def test_every_witness_was_launched(bench):
    table = W.witness_table()
    assert {k[:3] for k in table} == set(GROUPS)
    for key in sorted(table):   # (whatever an earlier test of this module has not run yet, e.g. when this test is selected alone)
        if key not in LAUNCHED:
            run_case(bench, table[key], key[3], key)
    assert set(LAUNCHED) == set(table)
    names = sorted({k[3] for k in LAUNCHED})
    print(len(names), "kernel names launched:", " ".join(names))
    assert len(names) == 28 + 23 + 6 + 1 + 28


def test_the_cases_beside_the_witnesses(bench):
    """More than one Cin block, lists of more than 1,024 rules (k_spconv_wgrad2<3,6,6,1> on the 15^3 block: three chunks of 1,152
    rows), k_wgrad_run with all four wave slots full and with LDS above 64 KB, operands at 4-byte boundaries."""
    names = [run_case(bench, case) for case in W.EXTRAS]
    assert all(no_rules(bench, case) for case in W.EXTRAS if case[3] < 336)
    assert "k_spconv_wgrad2<3,6,6,1>" in names and "k_wgrad_run<4,7>" in names and "k_spconv_wgrad<2,2>" in names


def test_swapped_run_lists_equal_the_table_entry_on_the_stride_2_table(bench):
    """mopa_spconv_bwd_weight_run with swap = 1 on the deconvolution table computes the stride-2 convolution's gradient: equal to
    mopa_spconv_bwd_weight on that convolution's own table within the bound the run-list test of tests/test_gpu_3d.py uses, and to
    float64 (run_case above); every NT and MU on `mixed` (two levels), `block8` and `two`."""
    table = W.witness_table()
    worst = 0.0
    for key in group_keys((1, 8, 1)):
        case = W.sliced(table[key])
        _, K, rows, cin, cout, v, one = case
        n = K * cin * cout
        for geom, level in (("mixed", 0), ("mixed", 1), ("block8", 0), ("two", 0)):
            _, flat, _, _ = bench.launch(case, geom, "up", level, 1)
            hit = bench.case(geom, "ch", level, cin, cout)
            own = bench.own_choice(geom, "ch", level, cin, cout)
            d = float((flat[W.TAIL + 1:W.TAIL + 1 + n] - own).abs().max()) / (2e-5 * hit["scale"])
            worst = max(worst, d)
            assert d <= 1, (case, geom, level, d)
    print(f"swap = 1 against the table entry: worst difference {worst:.3f} of 2e-5 max(1, max|ref|)")


def test_stem_and_the_simple_kernel_on_the_same_shape(bench):
    """1 -> 16 through k_spconv_stem_wgrad, and through k_spconv_wgrad<1,1> when dout starts at a 4-byte boundary."""
    table = W.witness_table()
    for K in (8, 27):
        stem, simple = table[(0, K, 0, "k_spconv_stem_wgrad<16>")], table[(0, K, 0, "k_spconv_wgrad<1,1>")]
        assert stem[3:5] == (1, 16) and W.TABLE_VARIANTS[stem[5]][3] == 0
        case = (0, K, 0, 1, 16, 4, 0)
        assert W.TABLE_VARIANTS[4][3] == 4 and run_case(bench, case) == "k_spconv_wgrad<1,1>"
        assert run_case(bench, (0, K, 0, 1, 16, 0, 0)) == "k_spconv_stem_wgrad<16>"   # (ld 9 / 24 at column 4, and on `mixed` ld 1 / 16)
        assert W.sliced((0, K, 0, 1, 16, 0, 0))[5] == 8 and W.TABLE_VARIANTS[8][:2] == (8, 8)
        assert run_case(bench, (0, K, 0, 1, 16, 2, 0)) == "k_spconv_wgrad<1,1>"   # ld_dout % 4 != 0


def test_refusals_launch_nothing(bench):
    from mopa_amd._lib import call, ptr, query, stream
    tab = bench.table("mixed", "nbr27", 0)
    K, A = tab.shape
    runs = bench.runs("mixed", "nbr27", 0)
    x = torch.zeros(A * 280 + 8, device="cuda")
    g = torch.zeros(A * 128 + 8, device="cuda")
    dw = torch.full((27 * 272 * 128,), W.SENTINEL, device="cuda")
    ws = torch.full((query("mopa_spconv_wgrad_workspace_bytes", K, A, 272, 112) // 4 + 64,), W.SENTINEL, device="cuda")

    def table(cin, cout, ld_in=280, ld_do=128, ws_bytes=4 * ws.numel(), acc=0):
        call("mopa_spconv_bwd_weight", ptr(tab), K, A, ptr(x), ld_in, cin, ptr(g), ld_do, cout, ptr(dw), acc, ptr(ws), ws_bytes, stream())

    def run(cin, cout, ld_in=280, ld_do=128, xcol=0, gcol=0, wcol=0, ws_bytes=4 * ws.numel() - 16, acc=0):
        call("mopa_spconv_bwd_weight_run", ptr(runs), K, A, 0, 0, ptr(x, xcol), ld_in, cin, ptr(g, gcol), ld_do, cout, ptr(dw), acc, ptr(ws, wcol),
             ws_bytes, stream())

    arg = [lambda: table(16, 128), lambda: table(16, 16, ld_in=15), lambda: table(16, 16, ld_do=12), lambda: run(16, 16, ld_in=278),
           lambda: run(16, 16, ld_do=126), lambda: run(16, 16, xcol=1), lambda: run(16, 16, gcol=2), lambda: run(16, 16, wcol=1),
           lambda: run(272, 16), lambda: run(8, 16), lambda: run(16, 128), lambda: run(16, 16, ld_do=12)]
    need_t = W.ask(0, K, A, 64, 32, 0, 0)[1][W.I_WS]
    need_r = W.ask(1, K, A, 64, 32, 0, 0)[1][W.I_WS]
    big = W.stated(64 * 4100)   # a stated size that asks for more chunks than the table's own plan
    need_big = W.ask(0, K, A, 64, 32, 0, 0, big)[1][W.I_WS]
    assert need_t == query("mopa_spconv_wgrad_workspace_bytes", K, A, 64, 32) and need_r == query("mopa_spconv_wgrad_run_workspace_bytes", K, A, 64, 32, 0)
    assert need_big >= need_t
    short = [lambda: table(64, 32, ws_bytes=need_t - 4), lambda: run(64, 32, ws_bytes=need_r - 4), lambda: table(64, 32, ws_bytes=need_big - 4, acc=big),
             lambda: run(64, 32, ws_bytes=W.ask(1, K, A, 64, 32, 0, 0, W.stated(64 * 20000))[1][W.I_WS] - 4, acc=W.stated(64 * 20000))]
    for f in arg:
        with pytest.raises(RuntimeError, match="code -1"):
            f()
    for f in short:
        with pytest.raises(RuntimeError, match="code -2"):
            f()
    torch.cuda.synchronize()
    assert (dw == W.SENTINEL).all() and (ws == W.SENTINEL).all()
    table(64, 32, ws_bytes=need_t)      # (the calls the refusals are one step away from)
    run(64, 32, ws_bytes=need_r)
    table(64, 32, ws_bytes=need_big, acc=big)
    torch.cuda.synchronize()
    assert (dw[:K * 64 * 32] != W.SENTINEL).all() and (dw[K * 64 * 32:] == W.SENTINEL).all()
    assert (ws[max(need_t, need_r, need_big) // 4:] == W.SENTINEL).all()
