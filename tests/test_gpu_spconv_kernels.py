"""Every forward kernel of the sparse convolution (csrc/spconv.hip, csrc/sprun.hip) on geometries of under 800 rows against
oracle.scn3d.sparse_conv in float64.  Run with -m gpu on an MI355X.

The dispatch picks an instantiation from the channel pair and the table's row count; bits 8-30 of w_flip state another row count for
that choice alone, so the kernels of the quarter-million-row levels run here on tables of 1 to 786 rows: tiles of 3 and of 108
groups, two and three metadata chunks, a tile of exactly two chunks, fewer groups than waves, a last tile of 9 rows, a table of one
row, and tables that start and end inside the shared group arrays (tests/_spconv_cases.py; tests/test_spconv_picks_host.py computes
the witness table and shows that single defects exceed the bound tenfold).  Per launch: the query names the witness's kernel, the
result is within rtol 1e-4 / atol 2e-5 max(1, max|ref|) (the forward bounds of tests/test_gpu_3d.py), the input is a slice of a
buffer of NaN, the output a slice of a buffer of sentinels with 64 sentinel rows behind it, a second launch gives the same bits, and
mopa_spconv_fwd_run gives the bits of mopa_spconv_fwd (the same MFMA operand mapping, offsets ascending) for both RG
and every NT.  Bit identity of the other kernels with the dense-table kernel is observed and printed, not asserted: k_spconv_pipe /
k_spconv_t4 add a group's product chunk by chunk (see the comment above k_spconv_pipe)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _spconv_cases as C

pytestmark = pytest.mark.gpu

CHUNK = 24
CHUNKS = [(e, K, i) for e, K, n in ((0, 8, 2), (0, 27, 2), (1, 8, 4), (1, 27, 4), (2, 8, 2), (2, 27, 1)) for i in range(n)]
LAUNCHED = {}   # witness key -> (launches, worst error / bound, worst error / max|ref|, launches with the dense-table kernel's bits, compared)


@pytest.fixture(scope="module")
def bench():
    return C.Bench3D()


def chunk_keys(entry, K, i):
    keys = sorted(k for k in C.witness_table() if k[:2] == (entry, K))
    return keys[i * CHUNK:(i + 1) * CHUNK]


def run_witness(bench, key, transposed=False, geometries=C.GEOMETRIES):
    entry, K, name = key
    case = C.witness_table()[key]
    vecs = []
    for geom in geometries:
        for kind, level, flip in C.tables_of(geom, K, case[7] if entry == 2 else None):
            if transposed and not (flip or kind == "up"):   # backward-data runs on the reversed table
                continue
            kname, v = bench.measure(case, geom, kind, level, flip, transposed)
            assert kname == name, (case, geom, kind, level)     # the right kernel
            vecs.append(v)
    m = torch.stack(vecs).cpu().numpy()
    compared = m[:, 4] >= 0
    print(f"{C.ENTRIES[entry]} K {K} {name}{' (backward-data)' if transposed else ''}: {len(m)} launches, worst error {m[:, 0].max():.3f} of the bound, "
          f"{m[:, 1].max():.2e} of max|ref|, dense-table bits in {int((m[:, 4] == 1).sum())} of {int(compared.sum())}")
    assert (m[:, 0] <= 1).all(), (case, m[:, 0].max())          # accuracy
    assert (m[:, 2] == 1).all(), case                           # every sentinel untouched
    assert (m[:, 3] == 1).all(), case                           # determinism
    if entry == 2:
        assert compared.all() and (m[:, 4] == 1).all(), case    # mopa_spconv_fwd's bits
    if not transposed:
        LAUNCHED[key] = (len(m), float(m[:, 0].max()), float(m[:, 1].max()), int((m[:, 4] == 1).sum()), int(compared.sum()))


def test_geometries_are_the_cases_the_kernels_need(bench):
    from test_gpu_3d import _assert_geometry_equal
    for name in C.GEOMETRIES:
        g, o = bench.g[name], C.oracle_geometry(name)
        if o.num_active[0] > 1:
            _assert_geometry_equal(g, o)
        else:   # (that helper samples rows 0 and 1: the tables of the one-voxel geometry are compared here)
            assert g.num_active == o.num_active and np.array_equal(g.point_row.cpu().numpy(), o.point_row)
            for kind in ("nbr27", "ch", "up", "parent"):
                assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(getattr(g, kind), getattr(o, kind))), kind
        assert tuple(o.num_active) == C.EXPECT_ROWS[name] and max(o.num_active) < 800
        start = 0   # every table's groups lie behind those of the tables before it in the shared arrays; the last one ends at G
        for kind in ("nbr27", "ch", "up"):
            for level, (tg, to) in enumerate(zip(getattr(g, kind), getattr(o, kind))):
                groups = C.tile_groups(to)
                if (name, kind, level) in C.EXPECT_GROUPS:
                    assert groups == C.EXPECT_GROUPS[(name, kind, level)], (name, kind, level, groups)
                gs = g.rulebook(tg)[0].cpu().numpy()
                assert np.array_equal(gs, start + np.concatenate([[0], np.cumsum(groups)])), (name, kind, level)
                start = int(gs[-1])
        assert start > 0
    o = C.oracle_geometry("block8")
    assert C.tile_groups(o.nbr27[0])[:2] == (72, 108) and max(C.tile_groups(o.nbr27[0])) == 27 * 4
    assert (np.asarray(C.oracle_geometry("one").nbr27[0]) >= 0).sum() == 1


@pytest.mark.parametrize("entry,K,i", CHUNKS)
def test_witnesses_vs_float64(bench, entry, K, i):
    for key in chunk_keys(entry, K, i):
        run_witness(bench, key)


def test_every_witness_was_launched(bench):
    table = C.witness_table()
    assert all(len([k for k in table if k[:2] == (e, K)]) <= CHUNK * len([c for c in CHUNKS if c[:2] == (e, K)]) for e, K, _ in CHUNKS)
    for key in sorted(table):   # (whatever an earlier test of this module has not run yet, e.g. when this test is selected alone)
        if key not in LAUNCHED:
            run_witness(bench, key)
    assert set(LAUNCHED) == set(table)
    assert len({k[2] for k in LAUNCHED}) == len({k[2] for k in table}) and len(LAUNCHED) == len(table)


def test_backward_data_weight_forms_one_witness_per_family(bench):
    """The layer's weight [K][cout][cin] packed with transpose = 1 (mopa_spconv_pack_weight, mopa_spconv_run_pack_weight,
    mopa_spconv_transpose_weight) on the reversed table: mirrored offsets of the 27-offset table, the deconvolution table."""
    table = C.witness_table()
    done = set()
    for key in sorted(table, key=lambda k: (-table[k][3], k)):   # (the widest input first: more than one chunk per unit)
        fam = (key[0], key[1], key[2].split("<")[0])
        if fam in done or (key[0] == 2 and key[1] == 8 and not table[key][7]) or "stem" in key[2]:
            continue
        done.add(fam)
        run_witness(bench, key, transposed=True, geometries=("mixed", "block8"))
    assert {f[2] for f in done} == {"k_spconv_fwd", "k_spconv_blk", "k_spconv_pipe", "k_spconv_t4", "k_spconv_run"}


def test_refusals_launch_nothing(bench):
    from mopa_amd._lib import call, ptr, query, stream
    g = bench.g["mixed"]
    tab = g.nbr27[0]
    K, A = tab.shape
    gs, go, gi, gout = g.rulebook(tab)
    runs, _ = bench.runs("mixed", "nbr27", 0)
    big = C.stated(64 * 4096)
    out = torch.full((A + C.GUARD_ROWS, 256), C.SENTINEL, device="cuda")
    x = torch.zeros(A, 264, device="cuda")
    w = torch.zeros(27 * 240 * 240 + 4, device="cuda")
    ws = torch.empty(query("mopa_spconv_run_workspace_bytes", K, A, 16) // 4, device="cuda")

    def grouped(cin, cout, flags, ld_in=264, wcol=0):
        call("mopa_spconv_fwd_grouped", ptr(gs), ptr(go), ptr(gi), ptr(gout), K, A, ptr(x), ld_in, cin, ptr(w, wcol), cout, flags, ptr(out), 256,
             0, 0, stream())

    def run(cin, cout, ld_in=264, ws_bytes=4 * ws.numel()):
        call("mopa_spconv_fwd_run", ptr(runs), K, A, ptr(x), ld_in, cin, ptr(w), cout, 0, ptr(out), 256, 0, ptr(ws), ws_bytes, stream())

    assert C.pick_of(1, K, A, 16, 16, 264, big | 2) > 0
    grouped(16, 16, big | 2)   # (the call the refusals below are one step away from)
    out.fill_(C.SENTINEL)
    refused = [lambda: grouped(16, 16, big | 2, wcol=1),            # packed weights at an unaligned pointer
               lambda: grouped(16, 16, big | 2, ld_in=263),         # ld_in % 4 != 0
               lambda: run(16, 16, ld_in=263),
               lambda: grouped(240, 16, big | 2),                   # 240 input channels
               lambda: grouped(240, 16, big),
               lambda: run(240, 16),
               lambda: call("mopa_spconv_fwd", ptr(tab), K, A, ptr(x), 264, 240, ptr(w), 16, big, ptr(out), 256, stream()),
               lambda: grouped(16, 16, 2)]                          # packed weights where the plan says block kernel (7 tiles)
    assert C.pick_of(1, K, A, 16, 16, 264, 2) == -1 and query("mopa_spconv_grouped_wants_packed", K, A, 16, 16) == 0
    for f in refused:
        with pytest.raises(RuntimeError, match="code -1"):
            f()
    with pytest.raises(RuntimeError, match="code -2"):              # a slab one float short
        run(16, 16, ws_bytes=4 * ws.numel() - 4)
    run(16, 16)
    torch.cuda.synchronize()
    assert (out[:A, :16] != C.SENTINEL).all() and (out[:, 16:] == C.SENTINEL).all() and (out[A:] == C.SENTINEL).all()
    out.fill_(C.SENTINEL)
    for f in refused:
        with pytest.raises(RuntimeError):
            f()
    assert (out == C.SENTINEL).all()


def test_wide_pipelined_kernels_in_a_child_process():
    """MOPA_SPCONV_PATH=1 is read once per process: the worker runs k_spconv_pipe<2,6,32>, <3,6,40> and <4,4,28> with the same
    assertions (one child process; it prints the worst error per kernel)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_spconv_path_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, MOPA_SPCONV_PATH="1"), timeout=300, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:]
    for name in ("k_spconv_pipe<2,6,32>", "k_spconv_pipe<3,6,40>", "k_spconv_pipe<4,4,28>"):
        assert name + ":" in r.stdout
