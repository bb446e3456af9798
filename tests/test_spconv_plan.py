"""mopa_spconv_plan / mopa_spconv_wgrad_plan / mopa_rulebook_runs_wanted (csrc/scn_exec.hip, csrc/sprun.hip) are the one place where
the measured leaf rules (mopa_spconv_run_wanted, mopa_spconv_run_form, mopa_spconv_grouped_wants_packed, mopa_spconv_wgrad_run_wanted)
are combined into what a sparse convolution runs as; the native executor and the per-layer walk of mopa_amd/sparse3d.py both ask them.
The specification below is the composition as both walks spelled it out before the plan existed (sparse3d.spconv_fwd + spconv_launch,
spconv_bwd_weight_of, the RUN_MAX_ROWS rule of the geometry builder), as a function of the leaf rules alone; the plan must equal it
over every table size around every threshold and every channel pair of the network.  (No GPU: pure host queries.)"""
import ast
import itertools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

KINDS = ("subm", "down", "up", "nin")
ROWS_8_SCANS = (257465, 193135, 103554, 49022, 19312, 6789, 2330)   # active rows per level of 8 scans (tests/test_host_logic.py)


def q(name, *a):
    from mopa_amd._lib import query
    return query(name, *a)


def programs():
    from mopa_amd import sparse3d
    return [sparse3d.program_for(types.SimpleNamespace(in_channels=1, m=16, num_planes=7, block_reps=1, residual_blocks=res, prefix="p."))
            for res in (False, True)]


def channel_pairs():
    pairs = {(1, 16), (4, 16), (24, 40)}
    for prog in programs():
        for op in prog.ops:
            if op[0] == "conv":
                pairs |= {(op[4].C, op[5].C), (op[5].C, op[4].C)}
    return sorted(pairs)


def row_counts(pairs):
    widest = max(2 * cin for cin, _ in pairs)
    guard = -(-(1 << 32) // (8 * widest * 4))       # first rows with rows * 8 * ld_in * 4 >= 2^32 at the widest ld_in
    assert (guard - 1) * 8 * widest * 4 < 1 << 32 <= guard * 8 * widest * 4
    return (64 * 199, 64 * 200, 64 * 1499, 64 * 1500, 8191, 8192, 220000, 220001, 40000, guard - 1, guard)


# ---- the specification: the bodies the two walks had, on the leaf rules alone
def spec_fwd(K, rows, cin, cout, ld_in, has_rb, has_runs, one):
    """-> (path, weight form, workspace bytes): sparse3d.spconv_fwd + spconv_launch + spconv_launch_run."""
    narrow = rows * 8 * ld_in * 4 < 1 << 32
    if has_runs and narrow and q("mopa_spconv_run_wanted", K, rows, cin, cout, one):
        return 3, 0x10000 | (q("mopa_spconv_run_form", cin, cout) << 8), 0 if one else q("mopa_spconv_run_workspace_bytes", K, rows, cout)
    ntw = q("mopa_spconv_grouped_wants_packed", K, rows, cin, cout) if has_rb else 0
    if not narrow:
        ntw = 0
    if ntw > 0:
        return 2, ntw << 8, 0
    if has_rb and cin > 4 and (rows + 63) // 64 < (1500 if K == 27 else 200):
        return 1, 0, q("mopa_spconv_grouped_workspace_bytes", K, rows, cout)
    return 0, 0, 0


def spec_wgrad(kind, K, rows, has_runs, one, d_rows, d_has_runs, d_one, cin, cout):
    """-> (outcome, workspace bytes): sparse3d.spconv_bwd_weight_of."""
    if kind != "nin":
        r, swap = ((rows, one) if has_runs else None), 0
        if r is None and kind == "down":
            r, swap = ((d_rows, d_one) if d_has_runs else None), 1
            if r is not None and not r[1]:
                r = None
        if r is not None and q("mopa_spconv_wgrad_run_wanted", K, r[0], cin, cout, r[1]):
            return 1 + swap, q("mopa_spconv_wgrad_run_workspace_bytes", K, r[0], cin, cout, r[1])
    return 0, q("mopa_spconv_wgrad_workspace_bytes", K, rows, cin, cout)


def spec_runs_wanted(K, rows, one, mode=1):
    """Geometry3D.__init__: every deconvolution table, the 27-offset tables up to RUN_MAX_ROWS rows; nothing with MOPA_SPCONV_RUN=0."""
    return int(mode != 0 and (bool(one) or (K == 27 and rows <= 220000)))


def test_forward_plan_is_the_composition_of_the_leaf_rules():
    from mopa_amd.sparse3d import plan_parts
    pairs = channel_pairs()
    assert (192, 96) in pairs and (96, 192) in pairs and (32, 16) in pairs
    seen, n = set(), 0
    for K, rows, (cin, cout), wide, has_rb, has_runs, one in itertools.product((1, 8, 27), row_counts(pairs), pairs, (1, 2), (0, 1), (0, 1), (0, 1)):
        a = (K, rows, cin, cout, wide * cin, has_rb, has_runs, one)
        path, form, wsb = spec_fwd(*a)
        plan = q("mopa_spconv_plan", *a)
        assert plan_parts(plan) == (path, form), (a, hex(plan))
        assert q("mopa_spconv_plan_workspace_bytes", plan, K, rows, cout, one) == wsb, a
        seen.add(path)
        n += 1
    assert n == 3 * 11 * len(pairs) * 16 and seen == {0, 1, 2, 3}


def test_weight_gradient_plan_is_the_composition_of_the_leaf_rules():
    pairs = channel_pairs()
    seen = set()
    for kind, K, rows, (cin, cout), has_runs, one, d_rows, d_has_runs, d_one in itertools.product(
            range(4), (1, 8, 27), row_counts(pairs), pairs, (0, 1), (0, 1), (39999, 40000, 257465), (0, 1), (0, 1)):
        a = (K, rows, has_runs, one, d_rows, d_has_runs, d_one, cin, cout)
        want, wsb = spec_wgrad(KINDS[kind], *a)
        plan = q("mopa_spconv_wgrad_plan", kind, *a)
        assert plan == want, (KINDS[kind], a)
        t_rows, t_one = (d_rows, d_one) if plan == 2 else (rows, one)
        assert q("mopa_spconv_wgrad_plan_workspace_bytes", plan, K, t_rows, cin, cout, t_one) == wsb, (KINDS[kind], a)
        seen.add(plan)
    assert seen == {0, 1, 2}


def test_run_major_rulebooks_are_built_for_the_tables_the_rule_names():
    for K, rows, one in itertools.product((1, 8, 27), row_counts(channel_pairs()), (0, 1)):
        assert q("mopa_rulebook_runs_wanted", K, rows, one) == spec_runs_wanted(K, rows, one), (K, rows, one)
    assert q("mopa_rulebook_runs_wanted", 8, 515277, 1) == 1 and q("mopa_rulebook_runs_wanted", 8, 100, 0) == 0   # deconvolution / stride-2 convolution


@pytest.mark.parametrize("mode", [0, 2])
def test_run_major_rulebook_rule_follows_the_switch(mode):
    """MOPA_SPCONV_RUN is read once per process: 0 builds nothing, 2 (force the offset-major path) still nothing above 220,000 rows."""
    from mopa_amd import _lib
    cases = [(27, 220000, 0), (27, 220001, 0), (8, 515277, 1), (8, 100, 0)]
    code = ("import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); "
            f"print([lib.mopa_rulebook_runs_wanted(*c) for c in {cases!r}])")
    out = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH], env=dict(os.environ, MOPA_SPCONV_RUN=str(mode)), capture_output=True,
                         text=True, check=True).stdout
    assert ast.literal_eval(out.strip()) == [spec_runs_wanted(*c, mode=mode) for c in cases]


def fabricated_geometry(rows, with_runs):
    """A geom_host table (layout: csrc/scn_exec.hip) with real row counts and placeholder addresses: the size query reads the counts
    and which slots are set, and dereferences nothing."""
    L = len(rows)
    d = np.zeros(8 + 8 * (L + 1) + 8 + 24 + 8, np.int64)
    d[0:8] = (L, 4 * rows[0], 1, 1, 1, 1, 1, 1)
    for l in range(L):
        r = d[8 + 8 * l:16 + 8 * l]
        r[0:3] = (rows[l], 1, 1)
        tabs = [(27, rows[l], 0)]
        if l < L - 1:
            r[3:7] = 1
            tabs += [(8, rows[l + 1], 0), (8, rows[l], 1)]
        for i, (K, n, one) in enumerate(tabs):
            d[8 + 8 * (L + 1) + 8 + 3 * l + i] = int(with_runs and q("mopa_rulebook_runs_wanted", K, n, one))
            d[8 + 8 * (L + 1) + 8 + 24 + l] |= one << i
    return d


@pytest.mark.parametrize("with_runs", [True, False])
def test_native_workspace_covers_every_planned_launch_and_no_more_than_before(with_runs):
    from mopa_amd import _lib
    rows = ROWS_8_SCANS
    gd = fabricated_geometry(rows, with_runs)

    def table(kind, l, reversed_):   # -> (K, rows, grouped rulebook, run lists, one rule per row) as csrc/scn_exec.hip::table_of
        if kind == "subm":
            return 27, rows[l], 1, int(gd[8 + 64 + 8 + 3 * l]), 0
        if kind == "nin":
            return 1, rows[l], 0, 0, 0
        if (kind == "down") != reversed_:
            return 8, rows[l + 1], 1, int(gd[8 + 64 + 8 + 3 * l + 1]), 0
        return 8, rows[l], 1, int(gd[8 + 64 + 8 + 3 * l + 2]), 1

    for prog in programs():
        nt = prog.native_tables()
        got = int(_lib.load().mopa_scn_workspace_bytes(nt["prog"].ctypes.data, len(nt["prog"]), gd.ctypes.data, 10, 16))
        low = high = max(256, q("mopa_output_layer_heads_bwd_workspace_bytes", 4 * rows[0], 16, 10))
        for op in prog.ops:
            if op[0] == "bn":
                b = q("mopa_bnrelu_rows_bwd_workspace_bytes", rows[op[2].level], op[2].C)
                low, high = max(low, b), max(high, b)
            elif op[0] == "conv":
                _, _, kind, l, src, dst = op
                for rev in (False, True):
                    K, n, has_rb, has_runs, one = table(kind, l, rev)
                    cin, cout = (dst.C, src.C) if rev else (src.C, dst.C)
                    for ld_in in (cin, 2 * cin):
                        plan = q("mopa_spconv_plan", K, n, cin, cout, ld_in, has_rb, has_runs, one)
                        low = max(low, q("mopa_spconv_plan_workspace_bytes", plan, K, n, cout, one))
                    # before the plan: the block kernel's scratch for every table, the slab wherever the leaf rule wants the path
                    high = max(high, q("mopa_spconv_grouped_workspace_bytes", K, n, cout))
                    if has_runs and not one and q("mopa_spconv_run_wanted", K, n, cin, cout, 0):
                        high = max(high, q("mopa_spconv_run_workspace_bytes", K, n, cout))
                K, n, _, has_runs, one = table(kind, l, False)
                _, d_n, _, d_has_runs, d_one = table(kind, l, kind == "down")
                wplan, wsb = spec_wgrad(kind, K, n, has_runs, one, d_n, d_has_runs, d_one, src.C, dst.C)
                assert q("mopa_spconv_wgrad_plan", KINDS.index(kind), K, n, has_runs, one, d_n, d_has_runs, d_one, src.C, dst.C) == wplan
                low, high = max(low, wsb), max(high, wsb)
        assert low <= got <= high, (low, got, high)
