"""Parity of the HIP 3D path (through the C-ABI) against the CPU oracle.  Run with -m gpu on an MI355X.

Integer work (hash, active sets, rule tables): bit-exact.  fp32 features: rtol 1e-4 / atol 1e-5 per layer,
end-to-end logits atol 1e-3 (SURVEY.md 8c "Tolerances").
"""
import numpy as np
import pytest
import torch

from oracle import scn3d
from oracle.params import det_state

pytestmark = pytest.mark.gpu


def _cloud(seed, n=3000, size=48, batch=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    # clustered points so that neighbourhoods are non-trivial and duplicates occur
    centers = rng.integers(4, size - 4, (40, 3))
    c = centers[rng.integers(0, 40, n)] + rng.integers(-3, 4, (n, 3))
    c = np.clip(c, 0, size - 1)
    b = rng.integers(0, batch, (n, 1))
    return np.concatenate([c, b], 1).astype(np.int64)


def _geoms(coords, levels, full_scale):
    from mopa_amd.sparse3d import Geometry3D
    g = Geometry3D(torch.from_numpy(coords), levels, full_scale, "cuda")
    o = scn3d.Geometry(coords, levels, full_scale)
    return g, o


def _assert_geometry_equal(g, o):
    assert g.num_active == o.num_active
    assert np.array_equal(g.point_row.cpu().numpy(), o.point_row)
    for l in range(o.num_levels):
        assert np.array_equal(g.row_keys[l].cpu().numpy().astype(np.uint64), o.row_keys[l]), l
        assert np.array_equal(g.nbr27[l].cpu().numpy(), o.nbr27[l]), l
    for l in range(o.num_levels - 1):
        assert np.array_equal(g.parent[l].cpu().numpy(), o.parent[l]), l
        assert np.array_equal(g.ch[l].cpu().numpy(), o.ch[l]), l
        assert np.array_equal(g.up[l].cpu().numpy(), o.up[l]), l
    rs, rp = g.row_start.cpu().numpy(), g.row_points.cpu().numpy()
    assert rs[0] == 0 and rs[-1] == o.n_points
    for r in (0, 1, o.num_active[0] // 2, o.num_active[0] - 1):
        assert np.array_equal(rp[rs[r]:rs[r + 1]], np.nonzero(o.point_row == r)[0])


def test_geometry_bit_exact_random():
    for seed, levels, fs in ((0, 4, 64), (1, 3, 4096), (2, 1, 64)):
        c = _cloud(seed)
        if fs == 4096:
            c[:, :3] *= 60  # spread over the full 12-bit range
            c[:, :3] += _cloud(seed + 10)[:, :3] // 8
        g, o = _geoms(c, levels, fs)
        _assert_geometry_equal(g, o)


def test_geometry_bit_exact_synthetic_scan_and_pins(golden_dir):
    import json, os
    from mopa_amd import synth
    b = synth.make_batch(2)
    coords = b["x"][0].numpy()
    g, o = _geoms(coords, 7, 4096)
    _assert_geometry_equal(g, o)
    pins = json.load(open(os.path.join(golden_dir, "g7_synth_pins.json")))
    g0, _ = _geoms(coords[coords[:, 3] == 0], 7, 4096)
    assert g0.num_active == pins["0"]["active"] and g0.num_rules == pins["0"]["rules"]


def test_geometry_rejects_out_of_range():
    from mopa_amd.sparse3d import Geometry3D
    c = _cloud(3)
    c[5, 1] = 4096
    with pytest.raises(RuntimeError):
        Geometry3D(torch.from_numpy(c), 2, 4096, "cuda")
    with pytest.raises(RuntimeError):
        Geometry3D(torch.zeros(0, 4, dtype=torch.int64), 2, 4096, "cuda")
    # a voxel outside a field smaller than the key range: x, y, z < 4096, but not < full_scale
    c = _cloud(3)
    Geometry3D(torch.from_numpy(c), 2, 64, "cuda")
    for axis in range(3):
        c = _cloud(3)
        c[5, axis] = 64
        with pytest.raises(RuntimeError, match="full_scale"):
            Geometry3D(torch.from_numpy(c), 2, 64, "cuda")
    c[5, 2] = 63
    Geometry3D(torch.from_numpy(c), 2, 64, "cuda")


@pytest.mark.parametrize("cin,cout", [(1, 16), (16, 16), (32, 16), (48, 48), (64, 32), (80, 96), (192, 96), (96, 112),
                                      (112, 112), (16, 1), (3, 20)])
def test_spconv_fwd_wgrad_dgrad_vs_oracle(cin, cout):
    from mopa_amd import sparse3d as s3
    c = _cloud(4, n=5000)
    g, o = _geoms(c, 2, 64)
    dev = "cuda"
    rng = np.random.Generator(np.random.PCG64(cin * 1000 + cout))
    for table_name, tab_g, tab_o, A_in, flip_for_dgrad in (
            ("subm", g.nbr27[0], o.nbr27[0], o.num_active[0], None),
            ("down", g.ch[0], o.ch[0], o.num_active[0], g.up[0]),
            ("up", g.up[0], o.up[0], o.num_active[1], g.ch[0])):
        K, A_out = tab_o.shape
        x = torch.from_numpy(rng.standard_normal((A_in, cin), dtype=np.float32))
        w = torch.from_numpy(rng.standard_normal((K, cin, cout), dtype=np.float32) * 0.2)
        gout = torch.from_numpy(rng.standard_normal((A_out, cout), dtype=np.float32))
        xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
        ref = scn3d.sparse_conv(xr, tab_o, wr)
        (ref * gout.double()).sum().backward()
        # forward, reading x from / writing out to channel slices of wider buffers (JoinTable layout)
        pad_in = 4 * ((cin + 3) // 4) + 8
        xin = torch.zeros(A_in, pad_in, device=dev)
        col = 4 if cin % 4 == 0 else 0
        xin[:, col:col + cin] = x.to(dev)
        outb = torch.full((A_out, cout + 8), 7.0, device=dev)
        xv, ov = s3.View(xin, col, cin), s3.View(outb, 4 if cout % 4 == 0 else 0, cout)
        scale = max(1.0, float(ref.abs().max()))
        for rb in (None, g.rulebook(tab_g)):   # dense-table kernel and grouped-rulebook kernel
            assert rb is not None or True
            outb.fill_(7.0)
            s3.spconv_fwd(tab_g, xv, w.to(dev), ov, rb=rb)
            got = ov.dense().cpu()
            np.testing.assert_allclose(got.numpy(), ref.detach().float().numpy(), rtol=1e-4, atol=2e-5 * scale)
        assert (outb[:, ov.col + cout:] == 7.0).all()  # neighbours of the slice untouched
        # backward-weight
        dw = torch.empty(K, cin, cout, device=dev)
        gv = s3.View(gout.to(dev).contiguous())
        s3.spconv_bwd_weight(tab_g, xv, gv, dw)
        sw = max(1.0, float(wr.grad.abs().max()))
        np.testing.assert_allclose(dw.cpu().numpy(), wr.grad.float().numpy(), rtol=2e-4, atol=5e-5 * sw)
        # backward-data through the reversed rules
        wt = s3.spconv_transpose_weight(w.to(dev))
        dx = s3.new_view(A_in, cin, dev)
        if table_name == "subm":
            s3.spconv_fwd(tab_g, gv, wt, dx, w_flip=True, rb=g.rulebook(tab_g))
        else:
            s3.spconv_fwd(flip_for_dgrad, gv, wt, dx, rb=g.rulebook(flip_for_dgrad))
        sx = max(1.0, float(xr.grad.abs().max()))
        np.testing.assert_allclose(dx.dense().cpu().numpy(), xr.grad.float().numpy(), rtol=1e-4, atol=2e-5 * sx)
        # same through the layer-weight form (the op transposes / packs as its kernel needs)
        dx2 = s3.new_view(A_in, cin, dev)
        if table_name == "subm":
            s3.spconv_fwd(tab_g, gv, w.to(dev), dx2, w_flip=True, rb=g.rulebook(tab_g), w_transposed=True)
        else:
            s3.spconv_fwd(flip_for_dgrad, gv, w.to(dev), dx2, rb=g.rulebook(flip_for_dgrad), w_transposed=True)
        assert torch.equal(dx2.t, dx.t)


def _run_book_oracle(tab):
    """numpy restatement of the run-major rulebook (csrc/sprun.hip): per filter offset the valid rules in output-row order, every
    run padded to whole 128-slot items."""
    K, A = tab.shape
    seg, cnt, rin, rout = [0], [], [], []
    pos = np.full((K, A), -1, np.int32)
    for o in range(K):
        rows = np.nonzero(tab[o] >= 0)[0]
        pos[o, rows] = seg[-1] + np.arange(len(rows))
        padn = (-len(rows)) % 128
        rin += [tab[o, rows], np.full(padn, -1, np.int32)]
        rout += [rows.astype(np.int32), np.full(padn, -1, np.int32)]
        cnt.append(len(rows))
        seg.append(seg[-1] + len(rows) + padn)
    return np.asarray(seg), np.asarray(cnt), np.concatenate(rin), np.concatenate(rout), pos


def test_run_major_rulebook_bit_exact():
    """Integer structure of the offset-major path: header, slots, positions and padding equal the numpy restatement, for the
    27-offset table, both stride-2 tables, a one-row table and a table longer than one scan chunk."""
    from mopa_amd.sparse3d import Geometry3D
    from mopa_amd._lib import call, query, stream
    g, o = _geoms(_cloud(11, n=6000), 3, 64)
    g1, o1 = _geoms(np.array([[5, 5, 5, 0]], np.int64), 2, 64)
    from mopa_amd import synth
    gs, os_ = _geoms(synth.make_batch(1)["x"][0].numpy(), 2, 4096)
    cases = [(g.nbr27[0], o.nbr27[0]), (g.nbr27[2], o.nbr27[2]), (g.ch[0], o.ch[0]), (g.up[0], o.up[0]), (g.up[1], o.up[1]),
             (g1.nbr27[0], o1.nbr27[0]), (gs.nbr27[0], os_.nbr27[0])]
    bufs, rows = [], []
    for tg, _ in cases:
        K, A = tg.shape
        buf = torch.full((query("mopa_rulebook_runs_bytes", K, A) // 4,), -7, dtype=torch.int32, device="cuda")
        bufs.append(buf)
        rows.append((tg.data_ptr(), K, A, buf.data_ptr()))
    desc = np.asarray(rows, dtype=np.int64)
    call("mopa_rulebook_runs_build_batched", desc.ctypes.data, len(rows), stream())
    for (tg, to), buf in zip(cases, bufs):
        K, A = to.shape
        seg, cnt, rin, rout, pos = _run_book_oracle(to)
        b = buf.cpu().numpy()
        cap = (K * A + K * 128 + 127) // 128 * 128
        assert np.array_equal(b[:K + 1], seg) and np.array_equal(b[32:32 + K], cnt) and b[64] == seg[-1]
        n = seg[-1]
        assert n % 128 == 0 and n <= cap
        assert np.array_equal(b[128:128 + n], rin)
        assert np.array_equal(b[128 + cap:128 + cap + n], rout)
        assert np.array_equal(b[128 + 2 * cap:128 + 2 * cap + K * A].reshape(K, A), pos)
    # the geometry builds them for its deconvolution tables and the 27-offset tables
    assert all(g.runs(t) is not None and g.runs(t)[1] == 1 for t in g.up)
    assert all(g.runs(t) is not None and g.runs(t)[1] == 0 for t in g.nbr27)


@pytest.mark.parametrize("cin,cout", [(16, 16), (32, 16), (48, 48), (64, 32), (64, 128), (80, 96), (192, 96), (96, 112), (112, 224), (224, 112)])
def test_offset_major_convolution_equals_the_table_kernel_bit_for_bit(cin, cout):
    """mopa_spconv_fwd_run (run-major rulebook, per-offset GEMM, ordered per-row sum) against mopa_spconv_fwd on the same table:
    the same products (the same MFMA operand mapping) added in the same order (filter offsets ascending) -- identical bits, on the
    27-offset table (plain and with mirrored offsets = backward-data), the stride-2 convolution table (several rules per row) and
    the deconvolution table (one rule per row, products written straight to the output); and against the fp64 oracle."""
    from mopa_amd import sparse3d as s3
    from mopa_amd._lib import call, ptr, query, stream
    c = _cloud(5, n=7000)
    g, o = _geoms(c, 2, 64)
    dev = "cuda"
    rng = np.random.Generator(np.random.PCG64(cin * 977 + cout))
    for tab_g, tab_o, A_in, flip in ((g.nbr27[0], o.nbr27[0], o.num_active[0], 0), (g.nbr27[0], o.nbr27[0], o.num_active[0], 1),
                                     (g.ch[0], o.ch[0], o.num_active[0], 0), (g.up[0], o.up[0], o.num_active[1], 0)):
        K, A_out = tab_o.shape
        one = int(tab_g is g.up[0])
        x = torch.from_numpy(rng.standard_normal((A_in, cin), dtype=np.float32)).to(dev)
        w = torch.from_numpy(rng.standard_normal((K, cin, cout), dtype=np.float32) * 0.2).to(dev)
        xin = torch.zeros(A_in, cin + 8, device=dev)
        xin[:, 4:4 + cin] = x
        xv = s3.View(xin, 4, cin)
        ref_b = torch.full((A_out, cout + 8), 7.0, device=dev)
        rv = s3.View(ref_b, 4, cout)
        if cin <= 192:
            call("mopa_spconv_fwd", ptr(tab_g), K, A_out, xv.p, xv.ld, cin, ptr(w), cout, flip, rv.p, rv.ld, stream())
        runs = g.runs(tab_g)
        if runs is None:   # (the stride-2 convolution table gets none from the geometry: the dispatcher never sends it here)
            buf = torch.empty(query("mopa_rulebook_runs_bytes", K, A_out) // 4, dtype=torch.int32, device=dev)
            desc = np.asarray([(tab_g.data_ptr(), K, A_out, buf.data_ptr())], dtype=np.int64)
            call("mopa_rulebook_runs_build_batched", desc.ctypes.data, 1, stream())
            runs = (buf, 0)
        assert runs[1] == one
        wr = torch.empty_like(w)
        call("mopa_spconv_run_pack_weight", ptr(w), K, cin, cout, 0, ptr(wr), stream())
        out_b = torch.full((A_out, cout + 8), 7.0, device=dev)
        ov = s3.View(out_b, 4, cout)
        s3.spconv_launch_run(runs, K, xv, wr, ov, bool(flip))
        assert (out_b[:, :4] == 7.0).all() and (out_b[:, 4 + cout:] == 7.0).all()   # neighbours of the slice untouched
        if cin <= 192:
            assert torch.equal(ov.dense(), rv.dense()), (K, one, flip)
        wo = w.flip(0) if flip else w
        ref = scn3d.sparse_conv(x.cpu().double(), tab_o, wo.cpu().double())
        scale = max(1.0, float(ref.abs().max()))
        np.testing.assert_allclose(ov.dense().cpu().numpy(), ref.float().numpy(), rtol=1e-4, atol=2e-5 * scale)
        # the transposed form (backward-data packs the layer weight's per-offset transpose)
        wt = w.transpose(1, 2).contiguous()
        wr2 = torch.empty_like(w)
        call("mopa_spconv_run_pack_weight", ptr(wt), K, cout, cin, 1, ptr(wr2), stream())
        assert torch.equal(wr2, wr)
        # run to run: the same bits
        first = ov.dense().clone()
        s3.spconv_launch_run(runs, K, xv, wr, ov, bool(flip))
        assert torch.equal(first, ov.dense())


@pytest.mark.parametrize("cin,cout", [(16, 16), (48, 48), (64, 32), (80, 96), (128, 64), (160, 80), (192, 96), (224, 112)])
def test_weight_gradient_on_the_run_lists_vs_oracle_and_the_table_kernel(cin, cout):
    """mopa_spconv_bwd_weight_run (csrc/sprun.hip: pieces of equal rule count per filter offset, LDS-staged Cin x Cout GEMM, slabs
    summed in piece order) against the autograd of the fp64 oracle (oracle/scn3d.py::sparse_conv) and against the dense-table kernel
    mopa_spconv_bwd_weight: on the 27-offset table, on the deconvolution table (one rule per row) and -- lists swapped -- for the
    stride-2 convolution whose own table has no run-major rulebook; inputs as channel slices of wider buffers, the gradient written into
    a buffer that is only 4-byte aligned, accumulation onto a previous value, run to run the same bits (no atomics), and Cin values
    that leave some of the block's wave slots empty (80: blocks 2, 2, 1, 0)."""
    from mopa_amd import sparse3d as s3
    from mopa_amd._lib import call, ptr, query, stream
    c = _cloud(6, n=6000)
    g, o = _geoms(c, 2, 64)
    dev = "cuda"
    rng = np.random.Generator(np.random.PCG64(cin * 31 + cout))
    for name, tab_o, run_tab, one, swap, A_in in (("subm", o.nbr27[0], g.nbr27[0], 0, 0, o.num_active[0]),
                                                  ("up", o.up[0], g.up[0], 1, 0, o.num_active[1]),
                                                  ("down", o.ch[0], g.up[0], 1, 1, o.num_active[0])):
        K, A_out = tab_o.shape
        x = torch.from_numpy(rng.standard_normal((A_in, cin), dtype=np.float32))
        gout = torch.from_numpy(rng.standard_normal((A_out, cout), dtype=np.float32))
        wr = torch.zeros(K, cin, cout, dtype=torch.float64, requires_grad=True)
        (scn3d.sparse_conv(x.double(), tab_o, wr) * gout.double()).sum().backward()
        xin = torch.zeros(A_in, cin + 8, device=dev)
        xin[:, 4:4 + cin] = x.to(dev)
        gin = torch.zeros(A_out, cout + 8, device=dev)
        gin[:, 4:4 + cout] = gout.to(dev)
        xv, gv = s3.View(xin, 4, cin), s3.View(gin, 4, cout)
        runs = g.runs(run_tab)
        assert runs is not None and runs[1] == one
        Kr, Ar = run_tab.shape
        ws = torch.empty(query("mopa_spconv_wgrad_run_workspace_bytes", Kr, Ar, cin, cout, one), dtype=torch.uint8, device=dev)
        flat = torch.full((K * cin * cout + 2,), 3.0, device=dev)
        dw = flat[1:1 + K * cin * cout]                              # 4-byte aligned only
        prev = torch.from_numpy(rng.standard_normal(K * cin * cout).astype(np.float32)).to(dev)

        def run(acc):
            call("mopa_spconv_bwd_weight_run", ptr(runs[0]), Kr, Ar, one, swap, xv.p, xv.ld, cin, gv.p, gv.ld, cout, dw.data_ptr(), int(acc),
                 ptr(ws), ws.numel(), stream())

        run(False)
        got = dw.clone()
        assert float(flat[0]) == 3.0 and float(flat[-1]) == 3.0          # neighbours untouched
        sw = max(1.0, float(wr.grad.abs().max()))
        np.testing.assert_allclose(got.cpu().numpy().reshape(K, cin, cout), wr.grad.float().numpy(), rtol=2e-4, atol=5e-5 * sw, err_msg=name)
        run(False)
        assert torch.equal(dw, got), name                                # deterministic
        dw.copy_(prev)
        run(True)
        np.testing.assert_allclose((dw - prev).cpu().numpy(), got.cpu().numpy(), rtol=0, atol=2e-6 * sw + 1e-6 * float(prev.abs().max()))
        # the dense-table kernel on the layer's own table
        tab_g = {"subm": g.nbr27[0], "up": g.up[0], "down": g.ch[0]}[name]
        ref = torch.empty(K, cin, cout, device=dev)
        s3.spconv_bwd_weight(tab_g, xv, gv, ref)
        np.testing.assert_allclose(got.cpu().numpy().reshape(K, cin, cout), ref.cpu().numpy(), rtol=0, atol=2e-5 * sw, err_msg=name)


@pytest.mark.parametrize("n,batch", [(7, 1), (60, 2), (700, 3)])
def test_weight_gradient_on_the_run_lists_tiny_geometries(n, batch):
    """mopa_spconv_bwd_weight_run where pieces, tiles and filter offsets are mostly empty: 7 / 60 / 700 points (fewer rows than one
    32-slot tile; offsets without a single rule; runs that are all padding), 64 -> 48 and 80 -> 16 channels, every table kind -- against
    the dense-table kernel."""
    from mopa_amd import sparse3d as s3
    from mopa_amd._lib import call, ptr, query, stream
    c = _cloud(9 + n, n=n, size=24, batch=batch)
    g, o = _geoms(c, 2, 32)
    dev = "cuda"
    rng = np.random.Generator(np.random.PCG64(n))
    for cin, cout in ((64, 48), (80, 16)):
        for name, tab_g, run_tab, one, swap, A_in in (("subm", g.nbr27[0], g.nbr27[0], 0, 0, o.num_active[0]),
                                                      ("up", g.up[0], g.up[0], 1, 0, o.num_active[1]),
                                                      ("down", g.ch[0], g.up[0], 1, 1, o.num_active[0])):
            K, A_out = tab_g.shape
            x = torch.from_numpy(rng.standard_normal((A_in, cin), dtype=np.float32)).to(dev)
            gout = torch.from_numpy(rng.standard_normal((A_out, cout), dtype=np.float32)).to(dev)
            xv, gv = s3.View(x), s3.View(gout)
            ref = torch.empty(K, cin, cout, device=dev)
            s3.spconv_bwd_weight(tab_g, xv, gv, ref)
            runs = g.runs(run_tab)
            Kr, Ar = run_tab.shape
            ws = torch.empty(query("mopa_spconv_wgrad_run_workspace_bytes", Kr, Ar, cin, cout, one), dtype=torch.uint8, device=dev)
            dw = torch.full((K, cin, cout), float("nan"), device=dev)
            call("mopa_spconv_bwd_weight_run", ptr(runs[0]), Kr, Ar, one, swap, xv.p, xv.ld, cin, gv.p, gv.ld, cout, ptr(dw), 0, ptr(ws), ws.numel(), stream())
            scale = max(1.0, float(ref.abs().max()))
            np.testing.assert_allclose(dw.cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=2e-5 * scale, err_msg=f"{name} {cin}->{cout}")


def test_weight_gradient_dispatch_native_executor_equals_python_walk(monkeypatch):
    """The native executor (csrc/scn_exec.hip) and the Python walk (sparse3d.spconv_fwd / spconv_bwd_weight_of) ask the same plan per
    layer (mopa_spconv_plan, mopa_spconv_wgrad_plan: here the 64- to 192-channel 27-offset layers take the run lists for the weight
    gradient, the rest the dense table) and give the same bits for the three outputs, every parameter gradient and d(feats)."""
    from mopa_amd import sparse3d as s3, synth
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_3d
    batch = synth.make_batch(2, H=16, W=16)
    calls = []
    inner = s3.call
    monkeypatch.setattr(s3, "call", lambda name, *a: (calls.append(name), inner(name, *a))[1])

    def run(native):
        monkeypatch.setattr(s3, "NATIVE", native)
        torch.manual_seed(3)
        m = build_model_3d(default_cfg())[0].cuda().train()
        feats = batch["x"][1].cuda().requires_grad_()
        out = m(dict(batch, x=[batch["x"][0], feats]))
        g = torch.Generator(device="cuda").manual_seed(5)
        (out["seg_logit"] * torch.randn(out["seg_logit"].shape, device="cuda", generator=g)).sum().backward()
        torch.cuda.synchronize()
        assert feats.grad is not None and sorted(out) == ["feats", "seg_logit", "seg_logit2"]
        got = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        got.update({"out/" + k: v.detach().clone() for k, v in out.items()})
        got["d(feats)"] = feats.grad.clone()
        return got

    ga = run(True)
    n0 = calls.count("mopa_spconv_bwd_weight_run")
    gb = run(False)
    assert n0 == 0   # (native: one C-ABI call per pass)
    assert calls.count("mopa_spconv_bwd_weight_run") >= 5 and calls.count("mopa_spconv_bwd_weight") >= 10
    assert sorted(ga) == sorted(gb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_the_python_walk_launches_what_the_plan_names_vs_oracle(monkeypatch):
    """sparse3d.spconv_fwd and spconv_bwd_weight_of launch the entry point mopa_spconv_plan / mopa_spconv_wgrad_plan name -- every
    forward path (dense table, block kernel with its offset-split workspace, pipelined kernels on packed weights, offset-major with
    and without the slab) and every weight-gradient outcome this geometry reaches -- and the result is the fp64 oracle's
    (oracle/scn3d.py::sparse_conv).  20,000 points: the smallest cloud of this generator with a deconvolution table of 8,192 rows, from
    where the one-rule-per-row offset-major rule takes it."""
    from mopa_amd import sparse3d as s3
    from mopa_amd._lib import query
    c = _cloud(21, n=20000)
    g, o = _geoms(c, 2, 64)
    A0, A1 = o.num_active
    assert (A0, A1) == (15347, 6130)
    dev = "cuda"
    calls = []
    inner = s3.call
    monkeypatch.setattr(s3, "call", lambda name, *a: (calls.append((name, a)), inner(name, *a))[1])
    rng = np.random.Generator(np.random.PCG64(21))
    DENSE, BLOCK, PACKED, RUN = range(4)
    entry = {DENSE: "mopa_spconv_fwd", BLOCK: "mopa_spconv_fwd_grouped", PACKED: "mopa_spconv_fwd_grouped", RUN: "mopa_spconv_fwd_run"}
    for tab_g, tab_o, A_in, cin, cout, path in ((g.nbr27[0], o.nbr27[0], A0, 1, 16, DENSE), (g.ch[0], o.ch[0], A0, 32, 16, BLOCK),
                                                (g.nbr27[0], o.nbr27[0], A0, 64, 32, PACKED), (g.nbr27[0], o.nbr27[0], A0, 64, 64, RUN),
                                                (g.up[0], o.up[0], A1, 32, 16, RUN), (g.up[0], o.up[0], A1, 16, 16, DENSE)):
        K, A_out = tab_o.shape
        x = torch.from_numpy(rng.standard_normal((A_in, cin), dtype=np.float32))
        w = torch.from_numpy(rng.standard_normal((K, cin, cout), dtype=np.float32) * 0.2)
        ref = scn3d.sparse_conv(x.double(), tab_o, w.double())
        rb, runs = g.rulebook(tab_g), g.runs(tab_g)
        assert rb is not None and (runs is not None) == (K == 27 or tab_g is g.up[0])
        one = runs[1] if runs is not None else 0
        plan = query("mopa_spconv_plan", K, A_out, cin, cout, cin, 1, int(runs is not None), one)
        assert s3.plan_parts(plan)[0] == path, (K, cin, cout, plan)
        xv, ov = s3.View(x.to(dev)), s3.new_view(A_out, cout, dev)
        del calls[:]
        s3.spconv_fwd(tab_g, xv, w.to(dev), ov, rb=rb, runs=runs)
        launches = [(n, a) for n, a in calls if n in entry.values()]
        assert len(launches) == 1 and launches[0][0] == entry[path], (K, cin, cout, [n for n, _ in calls])
        a = launches[0][1]
        if path in (BLOCK, PACKED):     # w_flip bit 1 = packed weights; the block kernel gets its offset-split workspace
            assert bool(a[11] & 2) == (path == PACKED) and bool(a[14]) == (path == BLOCK)
        if path == RUN:                 # the slab, unless every output row has one rule
            assert a[11] == one and bool(a[12]) == (not one)
        scale = max(1.0, float(ref.abs().max()))
        np.testing.assert_allclose(ov.dense().cpu().numpy(), ref.float().numpy(), rtol=1e-4, atol=2e-5 * scale, err_msg=f"{K} {cin}->{cout}")
    for kind, tab_o, A_in, cin, cout, wplan in (("subm", o.nbr27[0], A0, 64, 64, 1), ("down", o.ch[0], A0, 16, 32, 0),
                                               ("nin", o.nbr27[0][13:14], A0, 16, 32, 0)):
        K, A_out = tab_o.shape
        x = torch.from_numpy(rng.standard_normal((A_in, cin), dtype=np.float32))
        gout = torch.from_numpy(rng.standard_normal((A_out, cout), dtype=np.float32))
        wr = torch.zeros(K, cin, cout, dtype=torch.float64, requires_grad=True)
        (scn3d.sparse_conv(x.double(), tab_o, wr) * gout.double()).sum().backward()
        dw = torch.empty(K, cin, cout, device=dev)
        del calls[:]
        s3.spconv_bwd_weight_of(g, kind, 0, s3.View(x.to(dev)), s3.View(gout.to(dev)), dw)
        names = [n for n, _ in calls if n.startswith("mopa_spconv_bwd_weight")]
        assert names == ["mopa_spconv_bwd_weight_run" if wplan else "mopa_spconv_bwd_weight"], (kind, names)
        sw = max(1.0, float(wr.grad.abs().max()))
        np.testing.assert_allclose(dw.cpu().numpy(), wr.grad.float().numpy(), rtol=2e-4, atol=5e-5 * sw, err_msg=kind)


def test_dispatcher_sends_the_matrix_bound_layers_to_the_offset_major_kernel():
    """mopa_spconv_run_wanted: the rule written in csrc/sprun.hip (measured table: profiles/r5_spconv_run.md)."""
    from mopa_amd._lib import query
    want = lambda *a: query("mopa_spconv_run_wanted", *a)
    assert want(8, 257465, 32, 16, 1) == 1 and want(8, 13907, 112, 96, 1) == 1 and want(8, 6789, 112, 96, 1) == 0   # deconvolution tables from 8,192 rows
    assert want(8, 49022, 64, 80, 0) == 0                                                 # stride-2 convolution tables: never
    assert want(27, 49022, 128, 64, 0) == 1 and want(27, 98000, 64, 64, 0) == 1 and want(27, 19312, 80, 160, 0) == 1
    assert want(27, 386000, 64, 32, 0) == 0 and want(27, 98000, 64, 128, 0) == 0 and want(27, 103554, 48, 48, 0) == 0
    assert want(27, 257465, 16, 16, 0) == 0 and want(27, 2330, 20, 16, 0) == 0


@pytest.mark.parametrize("C,rows", [(16, 5000), (48, 777), (192, 300), (32, 1), (8, 4000), (12, 3000), (24, 2500), (36, 900), (72, 500)])
def test_bnrelu_rows_fwd_bwd_vs_oracle(C, rows):
    from mopa_amd import sparse3d as s3
    rng = np.random.Generator(np.random.PCG64(C + rows))
    x = torch.from_numpy(rng.standard_normal((rows, C), dtype=np.float32) * 3 + 5.0)
    gam = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32))
    bet = torch.from_numpy(rng.standard_normal(C).astype(np.float32))
    gout = torch.from_numpy(rng.standard_normal((rows, C), dtype=np.float32))
    for training in (True, False):
        if rows == 1 and training:
            continue
        rm, rv = torch.zeros(C) + 0.3, torch.ones(C) * 1.7
        xr, gr, br = x.double().requires_grad_(True), gam.double().requires_grad_(True), bet.double().requires_grad_(True)
        rmr, rvr = rm.double().clone(), rv.double().clone()
        ref = scn3d.bn_relu(xr, gr, br, rmr, rvr, training)
        (ref * gout.double()).sum().backward()
        dev = "cuda"
        xb = torch.zeros(rows, C + 16, device=dev)
        xb[:, 16:] = x.to(dev)
        xv = s3.View(xb, 16, C)
        yv = s3.new_view(rows, C, dev)
        stats = torch.empty(4, C, device=dev)
        rmd, rvd = rm.to(dev), rv.to(dev)
        s3.bnrelu_fwd(xv, yv, gam.to(dev), bet.to(dev), rmd, rvd, training, stats)
        np.testing.assert_allclose(yv.dense().cpu().numpy(), ref.detach().float().numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(rmd.cpu().numpy(), rmr.float().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rvd.cpu().numpy(), rvr.float().numpy(), rtol=1e-5, atol=1e-6)
        dx = s3.View(torch.ones(rows, C, device=dev))
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        s3.bnrelu_bwd(s3.View(gout.to(dev)), xv, dx, stats, training, dg, db, acc_dx=True)
        np.testing.assert_allclose(dx.dense().cpu().numpy() - 1.0, xr.grad.float().numpy(), rtol=1e-3, atol=2e-5)
        np.testing.assert_allclose(dg.cpu().numpy(), gr.grad.float().numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(db.cpu().numpy(), br.grad.float().numpy(), rtol=1e-4, atol=1e-4)


def _build_3d(num_planes, in_channels=1, C=5, dual=True, block_reps=1, residual=False, m=16):
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_3d
    cfg = default_cfg(C, dual)
    cfg.MODEL_3D.SCN.num_planes = num_planes
    cfg.MODEL_3D.SCN.in_channels = in_channels
    cfg.MODEL_3D.SCN.block_reps = block_reps
    cfg.MODEL_3D.SCN.residual_blocks = residual
    cfg.MODEL_3D.SCN.m = m
    model, _ = build_model_3d(cfg)
    sd = model.state_dict()
    model.load_state_dict({k: det_tensor_like(k, v) for k, v in sd.items()})
    return model.cuda()


def det_tensor_like(k, v):
    from oracle.params import det_tensor
    return det_tensor(k, v.shape)


def _oracle_run(model, coords, feats, num_planes, training, gouts, full_scale=4096, block_reps=1, dtype=torch.float64, residual=False, m=16):
    P = {k: v.detach().cpu().to(dtype).clone() for k, v in scn3d.fold_state_dict(model.state_dict()).items()}
    for k in P:
        if "running" not in k:
            P[k].requires_grad_(True)
    og = scn3d.Geometry(coords, num_planes, full_scale)
    f = feats.to(dtype).clone().requires_grad_(True)
    out = scn3d.net3dseg_forward(P, og, f, dual_head="linear2.weight" in P, training=training, num_planes=num_planes,
                                 block_reps=block_reps, residual_blocks=residual, m=m)
    if gouts is not None:
        sum((out[k] * gouts[k].to(dtype)).sum() for k in out).backward()
    return P, f, out


@pytest.mark.parametrize("num_planes,in_ch,reps,training,residual,seed", [(3, 1, 1, True, False, 7), (3, 4, 2, True, False, 7), (7, 1, 1, True, False, 7),
                                                                          (7, 1, 1, False, False, 8), (3, 1, 1, True, True, 7), (4, 2, 2, True, True, 8)])
def test_net3dseg_forward_backward_vs_oracle(num_planes, in_ch, reps, training, residual, seed):
    """residual=True: scn.UNet's ResNet-style blocks (ConcatTable(Identity | NetworkInNetwork, BN-SubM-BN-SubM) + AddTable),
    the `residual_blocks=True` constructor variant of mopa/models/scn_unet.py:14,28.  (The cloud seed is part of the case, see
    test_net3dseg_other_widths_vs_oracle: with the offset-major kernels of round 5 -- another summation order inside a row's
    product -- seed 7 of the last variant has ONE BatchNorm input within fp32 round-off of zero whose ReLU mask bit then differs
    from the fp64 pass; profiles/dbg_run_ab.py shows the two kernel families agree to 1e-6 on every tensor for the seeds without
    such an element and differ by exactly that one element's gradient otherwise.  The eval-mode case likewise: with the stem's scalar
    kernel of round 5 -- offsets added one after the other where the short-level block kernel summed three partial outputs -- seed 7
    has one such element, seeds 8-12 have none.)"""
    _check_net3dseg(num_planes, in_ch, reps, training, residual, seed=seed)


@pytest.mark.parametrize("m,num_planes,residual,seed", [(8, 7, False, 7), (12, 4, True, 8), (4, 3, False, 7), (32, 3, False, 9), (8, 4, True, 8)])
def test_net3dseg_other_widths_vs_oracle(m, num_planes, residual, seed):
    """UNetSCN(m) for widths other than the shipped 16 (mopa/models/scn_unet.py:11,23 accept any m; config/xmuda.py:219 ships 16):
    channel counts that are not multiples of 16 run the dense-table kernels, the output heads split a row over m/4 lanes rounded up
    to a power of two.  Same comparison as the m = 16 variants: fp64 oracle, fp32 oracle as the yardstick.  (The cloud seed is part of
    the case: on some clouds ONE activation sits within fp32 round-off of zero in front of a ReLU and its mask bit differs between the
    fp32 and the fp64 pass -- seed 7 for the residual variants, seeds 7 and 8 for m = 32: one element of one BatchNorm bias gradient off
    by that element's dy, everything else at 1e-6; profiles/dbg_width.py prints the per-parameter errors for any seed.)"""
    _check_net3dseg(num_planes, 1, 1, True, residual, m=m, seed=seed)


def _check_net3dseg(num_planes, in_ch, reps, training, residual, m=16, seed=7):
    torch.manual_seed(0)
    c = _cloud(seed, n=6000, size=120 if num_planes == 7 else 48)
    model = _build_3d(num_planes, in_ch, block_reps=reps, residual=residual, m=m)
    model.train(training)
    rng = np.random.Generator(np.random.PCG64(5))
    feats = torch.from_numpy(rng.random((c.shape[0], in_ch), dtype=np.float32) + 0.5)
    if not training:
        # well-conditioned eval case: running statistics := the batch statistics of this input (oracle pass with
        # momentum 1), otherwise arbitrary running stats blow activations up over 7 levels and ReLU-mask flips
        # dominate every fp32-vs-fp64 comparison.
        P0 = {k: v.detach().cpu().double().clone() for k, v in scn3d.fold_state_dict(model.state_dict()).items()}
        old, scn3d.BN_MOMENTUM = scn3d.BN_MOMENTUM, 1.0
        try:
            scn3d.net3dseg_forward(P0, scn3d.Geometry(c, num_planes), feats.double(), training=True,
                                   num_planes=num_planes, block_reps=reps, residual_blocks=residual, m=m)
        finally:
            scn3d.BN_MOMENTUM = old
        model.load_state_dict({k: v.float() for k, v in P0.items()})
    f_dev = feats.cuda().requires_grad_(True)
    sd_before = {k: v.clone() for k, v in scn3d.fold_state_dict(model.state_dict()).items()}
    out = model({"x": [torch.from_numpy(c), f_dev]})
    gouts = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape), dtype=np.float32)) for k, v in out.items()}
    sum((out[k] * gouts[k].cuda()).sum() for k in out).backward()
    model_ref = _build_3d(num_planes, in_ch, block_reps=reps, residual=residual, m=m)
    model_ref.load_state_dict(sd_before)
    P, f, ref = _oracle_run(model_ref, c, feats, num_planes, training, gouts, block_reps=reps, residual=residual, m=m)
    # yardstick: the same oracle in fp32 -- the HIP path (fp32) may differ from the fp64 truth by a small multiple of
    # what plain fp32 torch-CPU arithmetic differs by (summation-order noise grows with depth).
    model_ref.load_state_dict(sd_before)
    P32, f32, ref32 = _oracle_run(model_ref, c, feats, num_planes, training, gouts, block_reps=reps, dtype=torch.float32, residual=residual, m=m)

    def close(got, truth, yard, what):
        scale = max(1e-6, float(np.abs(truth).max()))
        err = float(np.abs(got - truth).max())
        yerr = float(np.abs(yard - truth).max())
        assert err <= max(4.0 * yerr, 2e-4 * scale), (what, err, yerr, scale)
        assert err <= 1e-2 * scale, (what, err, scale)

    for k in ("feats", "seg_logit", "seg_logit2"):
        close(out[k].detach().cpu().numpy(), ref[k].detach().numpy(), ref32[k].detach().double().numpy(), k)
    named = dict(model.named_parameters())
    for k, p in P.items():
        if p.requires_grad:
            close(named[k].grad.cpu().numpy(), p.grad.numpy(), P32[k].grad.double().numpy(), k)
    close(f_dev.grad.cpu().numpy(), f.grad.numpy(), f32.grad.double().numpy(), "dfeats")
    if training:  # running statistics were updated exactly like the oracle's
        sd = model.state_dict()
        for k in P:
            if "running" in k:
                np.testing.assert_allclose(sd[k].cpu().numpy(), P[k].float().numpy(), rtol=1e-4, atol=1e-5)


def test_net3dseg_equals_dense_network():
    """The HIP path against the SECOND, independent oracle (oracle/dense3d.py): the whole 7-level Net3DSeg executed as dense
    conv3d / conv_transpose3d / masked batch-norm on a 64^3 grid, driven by the reference's recorded layer graph (fixture G6) --
    no hashes, no row orders, no rule tables in the checker.  Logits, parameter gradients and running statistics; the yardstick is
    the same dense network in fp32 against itself in fp64."""
    from oracle import dense3d
    c, feats64 = dense3d.dense_case()
    feats = feats64.float()
    model = _build_3d(7).train()
    sd0 = {k: v.detach().cpu().clone() for k, v in scn3d.fold_state_dict(model.state_dict()).items()}
    rng = np.random.Generator(np.random.PCG64(5))
    f_dev = feats.cuda()
    out = model({"x": [torch.from_numpy(c), f_dev]})
    gouts = {k: torch.from_numpy(rng.standard_normal(tuple(out[k].shape), dtype=np.float32)) for k in ("seg_logit", "seg_logit2")}
    sum((out[k] * gouts[k].cuda()).sum() for k in gouts).backward()

    def dense(dtype):
        P = {k: v.to(dtype).clone() for k, v in sd0.items()}
        for k in P:
            if "running" not in k:
                P[k].requires_grad_(True)
        stats = {}
        o = dense3d.net3dseg_dense(P, c, feats.to(dtype), 64, stats=stats)
        sum((o[k] * gouts[k].to(dtype)).sum() for k in gouts).backward()
        return P, o, stats

    P, ref, stats = dense(torch.float64)
    P32, ref32, _ = dense(torch.float32)

    def close(got, truth, yard, what):
        scale = max(1e-6, float(np.abs(truth).max()))
        err, yerr = float(np.abs(got - truth).max()), float(np.abs(yard - truth).max())
        assert err <= max(4.0 * yerr, 2e-4 * scale), (what, err, yerr, scale)
        assert err <= 1e-2 * scale, (what, err, scale)

    for k in ("feats", "seg_logit", "seg_logit2"):
        close(out[k].detach().cpu().numpy(), ref[k].detach().numpy(), ref32[k].detach().double().numpy(), k)
    named = dict(model.named_parameters())
    for k, p in P.items():
        if p.requires_grad:
            g = named[k].grad.cpu().numpy().reshape(p.shape)
            close(g, p.grad.numpy(), P32[k].grad.double().numpy(), k)
    sd = scn3d.fold_state_dict(model.state_dict())
    for name, (mean, var, n) in stats.items():   # running = 0.9 * old + 0.1 * (batch mean, unbiased batch variance)
        np.testing.assert_allclose(sd[name + ".running_mean"].cpu().numpy(), (0.9 * sd0[name + ".running_mean"].double() + 0.1 * mean).numpy(),
                                   rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(sd[name + ".running_var"].cpu().numpy(),
                                   (0.9 * sd0[name + ".running_var"].double() + 0.1 * var * n / max(n - 1, 1)).numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("residual,needs_dfeats,wstream", [(False, False, False), (False, True, False), (True, True, False),
                                                          (False, False, True), (True, True, True)])
def test_native_executor_is_bit_identical_to_the_python_walk(residual, needs_dfeats, wstream, monkeypatch):
    """One C-ABI call per pass (csrc/scn_exec.hip) runs the same kernels in the same order as the per-layer walk from Python
    (kept for synchronised BatchNorm, MOPA_SCN_NATIVE=0): outputs, every parameter gradient, the input gradient and the running
    statistics are equal bit for bit -- two training steps, so the second pass re-uses / refreshes the derived weight forms.
    wstream: the executor's weight gradients on a second stream (MOPA_SCN_WGRAD_STREAM=1; the walk stays on one stream)."""
    from mopa_amd import sparse3d as s3
    from mopa_amd.optim import FlatAdam
    monkeypatch.setattr(s3, "SCN_WGRAD_STREAM", wstream)
    c = _cloud(17, n=9000, size=150)
    rng = np.random.Generator(np.random.PCG64(6))
    feats = torch.from_numpy(rng.random((c.shape[0], 1), dtype=np.float32) + 0.5)
    gouts = None
    results = []
    for native in (True, False):
        old = s3.NATIVE
        s3.NATIVE = native
        try:
            model = _build_3d(7 if not residual else 4, residual=residual).train()
            opt = FlatAdam(model.parameters(), lr=1e-3)
            run = []
            for step in range(2):
                opt.zero_grad()
                f = feats.cuda().requires_grad_(needs_dfeats)
                out = model({"x": [torch.from_numpy(c), f]})
                if gouts is None:
                    gouts = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape), dtype=np.float32)).cuda() for k, v in out.items()}
                sum((out[k] * gouts[k]).sum() for k in out).backward()
                run.append(({k: v.detach().clone() for k, v in out.items()}, opt.grad.clone(), None if f.grad is None else f.grad.clone()))
                opt.step()
            run.append({k: v.clone() for k, v in model.state_dict().items()})
            results.append(run)
        finally:
            s3.NATIVE = old
    a, b = results
    for step in range(2):
        for k in a[step][0]:
            assert torch.equal(a[step][0][k], b[step][0][k]), (step, k)
        assert torch.equal(a[step][1], b[step][1]), step
        assert (a[step][2] is None) == (b[step][2] is None) and (a[step][2] is None or torch.equal(a[step][2], b[step][2]))
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])


def test_net3dseg_duplicate_points_and_extra_feature_rows():
    # nuScenes quirk (Appendix B.8): more feature rows than coords; and every point duplicated once.
    c = _cloud(9, n=800, size=24)
    c = np.concatenate([c, c], 0)
    model = _build_3d(3).eval()
    feats = torch.ones(c.shape[0] + 37, 1)
    out = model({"x": [torch.from_numpy(c), feats]})
    _, _, ref = _oracle_run(model, c, feats, 3, False, None)
    r = ref["seg_logit"].detach().float().numpy()
    np.testing.assert_allclose(out["seg_logit"].detach().cpu().numpy(), r, rtol=1e-3, atol=1e-3 * max(1.0, np.abs(r).max()))
    assert out["feats"].shape == (c.shape[0], 16)
    half = c.shape[0] // 2
    assert torch.equal(out["feats"][:half], out["feats"][half:])


def test_device_voxelizer_bit_exact_with_reference(golden_dir):
    """G4: coords of augment_and_scale_3d (+ int64 cast, range filter) from the reference's rotated points."""
    import os
    from mopa_amd.voxelize import collate_scans, voxelize_scan
    from oracle.voxelize import voxel_coords
    g = dict(np.load(os.path.join(golden_dir, "g4_voxelize.npz")))
    for k in range(3):
        u = g[f"u{k}"] if bool(g[f"transl{k}"]) else None
        coords, keep = voxelize_scan(torch.from_numpy(g[f"aug_points{k}"]).cuda(), 20, 4096, u, batch_index=k)
        assert np.array_equal(coords[:, :3].cpu().numpy(), g[f"coords{k}"][g[f"keep{k}"]])
        assert np.array_equal(keep.cpu().numpy(), g[f"keep{k}"]) and bool((coords[:, 3] == k).all())
    # out-of-field points are dropped, full-size synthetic scan agrees with the oracle, collate layout
    from mopa_amd import synth
    pts = synth.lidar_points(3)
    big = pts.copy()
    big[:7] *= 400.0  # > 1 km away: outside the 4096-voxel field at 5 cm
    c, keep = voxelize_scan(torch.from_numpy(big).cuda(), 20)
    ci, kref = voxel_coords(big, 20)
    assert np.array_equal(keep.cpu().numpy(), kref) and np.array_equal(c[:, :3].cpu().numpy(), ci[kref]) and not kref.all()
    x = collate_scans([torch.from_numpy(synth.lidar_points(s)).cuda() for s in (0, 1)], 20)
    ref = synth.make_batch(2, H=8, W=8)["x"][0]
    assert torch.equal(x[0].cpu(), ref) and x[1].shape == (ref.shape[0], 1)


def test_device_rotation_stage_replays_the_reference_augmentation(golden_dir):
    """VERDICT r1 missing #4: the rotation / flip stage of augment_and_scale_3d on the device.  The matrix is drawn from
    numpy's global RNG exactly like the reference (same seed -> same matrix), applied in float32 on the GPU; the rotated
    points agree with the reference's to <= 2 ulp (its BLAS may fuse differently) and the voxel coordinates are the fixture's."""
    import os
    from mopa_amd.voxelize import draw_rotation, rotate_points, voxelize_scan
    g = dict(np.load(os.path.join(golden_dir, "g4_voxelize.npz")))
    for k in range(3):
        kw = dict(noisy_rot=0.1 * (k > 0), flip_y=0.5 * (k > 0), rot_z=6.2831 * (k > 1))
        np.random.seed(k)
        rot = draw_rotation(**kw)
        u = np.random.rand(3) if k > 0 else None
        if k > 0:
            assert np.allclose(u, g[f"u{k}"], rtol=0, atol=0)   # the replay consumed the RNG like the reference did
        pts = torch.from_numpy(g[f"points{k}"]).cuda()
        aug = rotate_points(pts, rot).cpu().numpy()
        ref = g[f"aug_points{k}"]
        assert np.abs(aug - ref).max() <= 2 * np.spacing(np.abs(ref).max().astype(np.float32))
        coords, keep = voxelize_scan(pts, 20, 4096, u, batch_index=0, rot=rot)
        want = g[f"coords{k}"][g[f"keep{k}"]]
        got = coords[:, :3].cpu().numpy()
        assert got.shape == want.shape and np.abs(got - want).max() <= 1   # a last-ulp difference can move a point across a voxel face
        assert (got == want).all(1).mean() >= 0.99
        assert rot is None or rot.dtype == np.float32


def test_cached_weight_forms_3d_follow_weight_updates_batched_and_single(monkeypatch):
    """The packed / transposed forms of the sparse-conv weights are cached per weight version and, after an update, ALL stale
    forms are rebuilt in one launch (mopa_spconv_pack_weights_batched).  Optimizer steps, a tracked in-place update and an EMA
    swap must all be seen, and the batched refresh must give the bits of the one-kernel-per-form path."""
    from mopa_amd import sparse3d, synth
    from mopa_amd.optim import FlatAdam
    from mopa_amd.pseudo import FlatEMA
    b = synth.make_batch(2, H=16, W=16)
    locs, feats = b["x"][0].cuda(), b["x"][1].cuda()

    def run(batched):
        monkeypatch.setattr(sparse3d, "BATCHED_REPACK", batched)
        sparse3d._weight_cache.clear()
        sparse3d._refreshed.clear()
        torch.manual_seed(0)
        m = _build_3d(7).train()
        opt = FlatAdam(m.parameters(), lr=1e-2)
        ema = FlatEMA(opt, decay=0.5)
        outs = []
        for it in range(3):
            opt.zero_grad()
            o = m({"x": [locs, feats]})
            (o["seg_logit"].square().mean() + o["seg_logit2"].square().mean()).backward()
            opt.step()
            ema.update()
            outs.append(o["seg_logit"].detach().clone())
        with torch.no_grad():
            first = m.net_3d.sparseModel_weights()[0] if hasattr(m.net_3d, "sparseModel_weights") else next(p for n, p in m.named_parameters() if p.dim() == 3)
            first.mul_(1.25)                                   # tracked in-place update of one cached layer
        m.eval()
        with torch.no_grad():
            outs.append(m({"x": [locs, feats]})["seg_logit"].clone())
            with ema.average_parameters():
                outs.append(m({"x": [locs, feats]})["seg_logit"].clone())
            outs.append(m({"x": [locs, feats]})["seg_logit"].clone())
        return outs

    a, s = run(True), run(False)
    for x, y in zip(a, s):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[3], a[4]) and torch.equal(a[3], a[5])


@pytest.mark.parametrize("native", [True, False])
def test_two_groups_of_scans_in_one_3d_pass_equal_two_calls(native, monkeypatch):
    """data_batch["bn_group_points"] = N0: the scans of two batches (source, target) go through Net3DSeg as ONE sparse tensor,
    BatchNorm statistics / running updates / gradients per group on row ranges (the first group's rows come first at every
    level: Geometry3D.split).  Against the two calls the reference makes (train_xmuda_mopa.py:343,427): the split row counts
    equal the first batch's own active-row counts at every level (integers, exact); logits, running statistics and parameter
    gradients agree to fp32 round-off (a row's sum is the same set of exact products in another order when its 64-row tile holds
    other rows; the weight gradient is one sum over both groups instead of two accumulated)."""
    from mopa_amd import sparse3d as s3
    from mopa_amd.sparse3d import Geometry3D
    monkeypatch.setattr(s3, "NATIVE", native)
    ca = _cloud(21, n=7000, size=130, batch=2)
    cb = _cloud(22, n=5000, size=130, batch=3)
    ca = ca[np.argsort(ca[:, 3], kind="stable")]   # scans in batch order, as collate builds them
    cb = cb[np.argsort(cb[:, 3], kind="stable")]
    cb2 = cb.copy()
    cb2[:, 3] += 2
    both = np.concatenate([ca, cb2])
    rng = np.random.Generator(np.random.PCG64(8))
    fa = torch.from_numpy(rng.random((len(ca), 1), dtype=np.float32) + 0.5).cuda()
    fb = torch.from_numpy(rng.random((len(cb), 1), dtype=np.float32) + 0.5).cuda()
    g = Geometry3D(torch.from_numpy(both), 7, 4096, "cuda", group_points=len(ca))
    ga = Geometry3D(torch.from_numpy(ca), 7, 4096, "cuda")
    assert [s[0] for s in g.split] == ga.num_active and all(0 < s[0] < a for s, a in zip(g.split, g.num_active))
    assert Geometry3D(torch.from_numpy(both), 7, 4096, "cuda").split is None
    # three groups: the boundaries are the row counts of the first and of the first two batches
    cc = _cloud(23, n=3000, size=130, batch=1)
    cc[:, 3] += 5
    three = np.concatenate([both, cc])
    g3 = Geometry3D(torch.from_numpy(three), 7, 4096, "cuda", group_points=[len(ca), len(both)])
    assert [s[0] for s in g3.split] == ga.num_active and [s[1] for s in g3.split] == g.num_active
    with pytest.raises(ValueError):
        Geometry3D(torch.from_numpy(three), 7, 4096, "cuda", group_points=[len(both), len(ca)])
    # the second batch NOT offset behind the first one's scan indices: its points fall into voxels of the first group -> refused
    # (checked on the device inside the geometry's one read-back), where the boundary would silently mix the BatchNorm groups
    with pytest.raises(ValueError, match="disjoint"):
        Geometry3D(torch.from_numpy(np.concatenate([ca, ca[:100]])), 7, 4096, "cuda", group_points=len(ca))

    def gout(shape, seed):
        return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape, dtype=np.float32)).cuda()

    two = _build_3d(7).train()
    outs = []
    for k, (c, f) in enumerate(((ca, fa), (cb, fb))):
        o = two({"x": [torch.from_numpy(c), f]})
        sum((o[n] * gout(tuple(o[n].shape), 100 * k + i)).sum() for i, n in enumerate(sorted(o))).backward()
        outs.append({n: v.detach().clone() for n, v in o.items()})
    one = _build_3d(7).train()
    o = one({"x": [torch.from_numpy(both), torch.cat([fa, fb])], "bn_group_points": len(ca)})
    na = len(ca)
    loss = 0
    for k, sl in enumerate((slice(0, na), slice(na, None))):
        loss = loss + sum((o[n][sl] * gout(tuple(o[n][sl].shape), 100 * k + i)).sum() for i, n in enumerate(sorted(o)))
    loss.backward()
    torch.cuda.synchronize()
    for k, sl in enumerate((slice(0, na), slice(na, None))):
        for n in outs[k]:
            ref, got = outs[k][n], o[n][sl]
            assert float((ref - got).abs().max()) <= 2e-5 * float(ref.abs().max()), (k, n)
    sa, sb = two.state_dict(), one.state_dict()
    for n in sa:
        assert float((sa[n] - sb[n]).abs().max()) <= 1e-5 * (float(sa[n].abs().max()) + 1e-6), n
    worst = 0.0
    for (n, p), (_, q) in zip(two.named_parameters(), one.named_parameters()):
        err = float((p.grad - q.grad).abs().max()) / (float(p.grad.abs().max()) + 1e-20)
        worst = max(worst, err)
        assert err <= 2e-4, (n, err)
    print("two calls vs one grouped pass: worst parameter-gradient difference / tensor max", worst)
    with pytest.raises(ValueError):
        one({"x": [torch.from_numpy(both), torch.cat([fa, fb])], "bn_group_points": len(ca), "geometry_3d": Geometry3D(torch.from_numpy(both), 7, 4096, "cuda")})


@pytest.mark.parametrize("native", [True, False])
def test_three_groups_of_scans_in_one_3d_pass_equal_three_calls(native, monkeypatch):
    """bn_group_points = [N0, N1]: source, target and the VGI batch of a MoPA iteration (train_xmuda_mopa.py:343,427,558) as one
    sparse tensor: same checks as for two groups, against three calls in that order."""
    from mopa_amd import sparse3d as s3
    monkeypatch.setattr(s3, "NATIVE", native)
    clouds = []
    import os
    # The cloud seeds are part of the case (as in test_net3dseg_other_widths_vs_oracle): a merged pass and three separate calls put a
    # row at different positions of the 64-row tiles, the output-stationary kernels then add its products in another order, and on
    # ~2 of 5 seed triples ONE BatchNorm input within fp32 round-off of zero gets another ReLU mask bit -- the stem's weight gradient
    # then differs by that row's share (1e-3).  Probed with MOPA_TEST_SEED3 = 31 (passed with the round-4 kernels, one flip with the
    # offset-major kernels of round 5), 34, 37, 43 (no flip), 40, 46 (one flip).
    s0 = int(os.environ.get("MOPA_TEST_SEED3", "34"))
    for k, (seed, n, nb) in enumerate(((s0, 6000, 2), (s0 + 1, 5000, 2), (s0 + 2, 4000, 2))):
        c = _cloud(seed, n=n, size=120, batch=nb)
        clouds.append(c[np.argsort(c[:, 3], kind="stable")])
    rng = np.random.Generator(np.random.PCG64(9))
    feats = [torch.from_numpy(rng.random((len(c), 1), dtype=np.float32) + 0.5).cuda() for c in clouds]
    merged = []
    for k, c in enumerate(clouds):
        c = c.copy()
        c[:, 3] += 2 * k
        merged.append(c)
    merged = np.concatenate(merged)
    cuts = [len(clouds[0]), len(clouds[0]) + len(clouds[1])]

    def gout(shape, seed):
        return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape, dtype=np.float32)).cuda()

    sep = _build_3d(7).train()
    outs = []
    for k, (c, f) in enumerate(zip(clouds, feats)):
        o = sep({"x": [torch.from_numpy(c), f]})
        sum((o[n] * gout(tuple(o[n].shape), 100 * k + i)).sum() for i, n in enumerate(sorted(o))).backward()
        outs.append({n: v.detach().clone() for n, v in o.items()})
    one = _build_3d(7).train()
    o = one({"x": [torch.from_numpy(merged), torch.cat(feats)], "bn_group_points": cuts})
    sls = (slice(0, cuts[0]), slice(cuts[0], cuts[1]), slice(cuts[1], None))
    loss = 0
    for k, sl in enumerate(sls):
        loss = loss + sum((o[n][sl] * gout(tuple(o[n][sl].shape), 100 * k + i)).sum() for i, n in enumerate(sorted(o)))
    loss.backward()
    torch.cuda.synchronize()
    for k, sl in enumerate(sls):
        for n in outs[k]:
            ref, got = outs[k][n], o[n][sl].detach()
            assert float((ref - got).abs().max()) <= 2e-5 * float(ref.abs().max()), (k, n)
    sa, sb = sep.state_dict(), one.state_dict()
    for n in sa:
        assert float((sa[n] - sb[n]).abs().max()) <= 1e-5 * (float(sa[n].abs().max()) + 1e-6), n
    for (n, p), (_, q) in zip(sep.named_parameters(), one.named_parameters()):
        assert float((p.grad - q.grad).abs().max()) <= 2e-4 * (float(p.grad.abs().max()) + 1e-20), n
