"""Every instantiation of conv2d.hip's implicit-GEMM body at shapes of a few hundred pixels, against the float64 restatement of its
index map (tests/_convgeom_reference.py, itself checked against torch by tests/test_convgeom_host.py).

pick_tile gives the MFMA path 64x64 below 200,000 output pixels, so the suite's other kernel-level convolution tests run that one
instantiation; the tile override of the public `flags` word (bits 8-15) reaches 256x64, 128x128 and 128x64 -- the tile of every
full-resolution layer -- at M = 1 ... 270, just under, at and over every tile edge.  Bounds: tests/test_gpu_2d.py::_close, forward
rtol 1e-4 / atol 2e-5 max|ref|, backward-data and weight gradients rtol 1e-3 / atol 1e-4 max|ref|.  The four MFMA tiles run
mfma_f32_32x32x2f32 over 16-deep chunks in the same tap, chunk, k order: identical bits.  The vector-pipe kernels
(MOPA_CONV2D_MFMA=0, read once per process) run in one child process: tests/_conv_vector_pipe_worker.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _conv_tiles_gpu as gt
import _convgeom_reference as cr

pytestmark = pytest.mark.gpu
MFMA = os.environ.get("MOPA_CONV2D_MFMA", "1") != "0"   # (0: the bit-identity and one-launch assertions below are skipped)
needs_mfma = pytest.mark.skipif(not MFMA, reason="MFMA kernels are switched off (MOPA_CONV2D_MFMA=0)")
IGEMM = "k_conv2d_igemm_mfma<%s>" if MFMA else "k_conv2d_igemm<%s>"


@pytest.fixture(scope="module", autouse=True)
def _worst_errors():
    yield
    gt.report()


@pytest.mark.parametrize("case", cr.igemm_cases(), ids=cr.case_id)
def test_igemm_every_tile(case):
    """mopa_conv2d_igemm on one operator geometry (all its classes) at tile overrides 1..4 and without: float64 within the bound,
    nothing written outside the class's own elements, accumulation onto a random previous value, the four tiles bit for bit."""
    P = cr.problem(*case)
    cout = cr.fields(P.geoms[0]).Cout
    for accumulate in (False, True):
        init = gt.initial_out(P, accumulate)
        ref, mask = gt.igemm_expect(P, init, accumulate)
        outs = {}
        for tile in (None, 0, 1, 2, 3):
            if tile == 1 and cout % 128:
                with pytest.raises(RuntimeError):
                    gt.run_igemm(P, tile, accumulate, init)
                continue
            outs[tile] = gt.run_igemm(P, tile, accumulate, init)
            gt.check_igemm(IGEMM % gt.TILES[3 if tile is None else tile], P, outs[tile], init, ref, mask)
        if MFMA:
            for tile, got in outs.items():
                assert torch.equal(got, outs[3]), (tile, float((got - outs[3]).abs().max()))


def test_igemm_refuses_what_it_cannot_run():
    from mopa_amd._lib import call, host_i32, ptr, stream
    P = cr.problem("conv3s1", (1, 5, 13), 64, 64, True)
    d = gt.device(P)
    out = gt.initial_out(P, False).cuda()
    good = dict(x=ptr(d.x, P.xcol), w=ptr(d.w), b=ptr(d.b), o=ptr(out, P.ocol), g=P.geoms[0], flags=0)

    def launch(**change):
        a = dict(good, **change)
        call("mopa_conv2d_igemm", a["x"], a["w"], a["b"], a["o"], ctypes.addressof(a["g"]), a["flags"], stream())

    launch()
    launch(flags=4 << 8)
    with pytest.raises(RuntimeError):
        launch(flags=2 << 8)                      # the 128x128 tile with 64 output channels
    with pytest.raises(RuntimeError):
        launch(flags=5 << 8)                      # there are four tiles
    for name in ("x", "w", "b", "o"):             # a pointer off by 4 bytes
        with pytest.raises(RuntimeError):
            launch(**{name: good[name] + 4})
    bad = host_i32(list(P.geoms[0]))
    bad[cr.FIELDS.index("ld_in")] += 2             # rows of 78 floats
    with pytest.raises(RuntimeError):
        launch(g=bad)
    torch.cuda.synchronize()
    assert bool((out[:, :P.ocol] == cr.OUT_SENTINEL).all())


# (kind, grid, Cin, Cout, bias): the equal classes of a transposed convolution; the stride-2 backward-data at 7x9 (4x5, 4x4, 3x5, 3x4
# pixels per image); the same at 15x23 with 3 images: 288, 264, 252, 231 rows = 2, 2, 1, 1 row tiles of 256, 3, 3, 2, 2 of 128 and
# 5, 5, 4, 4 of 64, and the class with the most taps (which the kernel starts first) is the shortest
CLASS_CASES = [("convt", (2, 9, 11), 64, 128, True), ("dgrad3s2", (2, 4, 5), 128, 64, False), ("dgrad3s2", (3, 8, 12), 64, 64, False)]


@needs_mfma
@pytest.mark.parametrize("case", CLASS_CASES, ids=cr.case_id)
def test_classes_one_launch_every_tile(case):
    """mopa_conv2d_igemm_classes (k_conv2d_igemm_mfma_classes<256,64>, <128,64>, <64,64>): the bits of four mopa_conv2d_igemm
    launches at the same tile, float64 within the bound, writing and accumulating."""
    P = cr.problem(*case)
    assert len(P.geoms) == 4
    if case[1] == (3, 8, 12):
        rows = [cr.fields(g).B * cr.fields(g).OHl * cr.fields(g).OWl for g in P.geoms]
        for bm in (256, 128, 64):
            assert -(-min(rows) // bm) < -(-max(rows) // bm)
    for accumulate in (False, True):
        init = gt.initial_out(P, accumulate)
        ref, mask = gt.igemm_expect(P, init, accumulate)
        for tile in (0, 2, 3):
            one = gt.run_igemm(P, tile, accumulate, init, classes=True)
            four = gt.run_igemm(P, tile, accumulate, init)
            assert torch.equal(one, four), (tile, accumulate, float((one - four).abs().max()))
            gt.check_igemm("k_conv2d_igemm_mfma_classes<%s>" % gt.TILES[tile], P, one, init, ref, mask)
    with pytest.raises(RuntimeError):
        gt.run_igemm(P, 1, False, init, classes=True)   # 128x128: never a classes kernel


@pytest.mark.parametrize("nbatch,cin", [(16, 48), (36, 16)])
@pytest.mark.parametrize("T", [1, 65, 257])
def test_igemm_batched_every_tile(nbatch, cin, T):
    """mopa_conv2d_igemm_batched on the flat geometry of wino_conv, strides that leave gaps: problem z is a single launch on the
    offset pointers bit for bit, and the float64 product."""
    from mopa_amd._lib import call, ptr, stream
    cout, ld_in, ld_out = 128, cin + 4, 128 + 8
    s_in, s_w, s_out = T * ld_in + 8, cin * cout + 4, T * ld_out + 12
    rng = np.random.Generator(np.random.PCG64(nbatch + T))
    x = torch.full((nbatch * s_in,), cr.IN_SENTINEL)
    w = torch.full((nbatch * s_w,), cr.IN_SENTINEL)
    ref = torch.full((nbatch * s_out,), cr.OUT_SENTINEL, dtype=torch.float64)
    mask = torch.zeros(nbatch * s_out, dtype=torch.bool)
    geom = cr.wino_geom(T, cin, cout, ld_in, ld_out)
    for z in range(nbatch):
        x[z * s_in:z * s_in + T * ld_in].reshape(T, ld_in)[:, :cin] = torch.from_numpy(rng.standard_normal((T, cin)).astype(np.float32))
        w[z * s_w:z * s_w + cin * cout] = torch.from_numpy(rng.standard_normal(cin * cout).astype(np.float32) * np.float32(0.05))
    for z in range(nbatch):
        sl = slice(z * s_out, z * s_out + T * ld_out)
        ref[sl] = cr.igemm_ref(geom, x[z * s_in:].double(), w[z * s_w:z * s_w + cin * cout].double().reshape(1, cin, cout), None,
                               ref[sl], False)
        mask[sl] = cr.touched(geom, T * ld_out)
    init = torch.full((nbatch * s_out,), cr.OUT_SENTINEL)
    xd, wd = x.cuda(), w.cuda()
    outs = {}
    for tile in (None, 0, 1, 2, 3):
        flags = gt.tile_flags(tile)
        out, single = init.cuda(), init.cuda()
        call("mopa_conv2d_igemm_batched", ptr(xd), ptr(wd), ptr(out), ctypes.addressof(geom), nbatch, s_in, s_w, s_out, flags, stream())
        for z in range(nbatch):
            call("mopa_conv2d_igemm", ptr(xd, z * s_in), ptr(wd, z * s_w), None, ptr(single, z * s_out), ctypes.addressof(geom), flags,
                 stream())
        outs[tile] = out.cpu()
        assert torch.equal(outs[tile], single.cpu()), tile
        assert torch.equal(outs[tile][~mask], init[~mask])
        g, r = outs[tile].double()[mask], ref[mask]
        assert gt.note(IGEMM % gt.TILES[3 if tile is None else tile] + " batched", (g - r).abs(), cr.bound(r, "fwd"), r) <= 1.0
    if MFMA:
        assert all(torch.equal(o, outs[3]) for o in outs.values())
    out = init.cuda()
    for bad in (dict(s_in=s_in + 2), dict(s_w=s_w + 1), dict(s_out=s_out + 6), dict(nbatch=65536)):
        a = dict(nbatch=nbatch, s_in=s_in, s_w=s_w, s_out=s_out)
        a.update(bad)
        with pytest.raises(RuntimeError):
            call("mopa_conv2d_igemm_batched", ptr(xd), ptr(wd), ptr(out), ctypes.addressof(geom), a["nbatch"], a["s_in"], a["s_w"],
                 a["s_out"], 0, stream())
    torch.cuda.synchronize()
    assert bool((out == cr.OUT_SENTINEL).all())


@pytest.mark.parametrize("case", cr.wgrad_cases(), ids=cr.case_id)
def test_bwd_weight_slices(case):
    """mopa_conv2d_bwd_weight at 1, 15, 16, 17, 257 and 513 pixels, the stem also at 1260 and 2349 (one short slice ... three slices, the
    last partly filled, slices that cross image rows and images): both output layouts, accumulation, two runs the same bits, a short
    workspace refused."""
    from mopa_amd._lib import query
    P = cr.problem(*case)
    g = cr.fields(P.geoms[0])
    # the slice count, from the workspace (one [taps][Cin][Cout] slab per slice, rounded up to 256 bytes); the stem's one-block MFMA
    # kernel takes 1152 pixels per slice, so it has two larger grids of its own for 2 and 3 slices
    slices = query("mopa_conv2d_wgrad_workspace_bytes", ctypes.addressof(P.geoms[0])) // (g.TH * g.TW * g.Cin * g.Cout * 4)
    M = g.B * g.OHl * g.OWl
    if MFMA and case[0] == "stem":
        assert slices == {1260: 2, 2349: 3}.get(M, 1)
    else:
        assert slices == {1: 1, 15: 1, 16: 1, 17: 1, 257: 2, 513: 3, 1260: 5, 2349: 10}[M]
    gt.check_wgrad(gt.wgrad_kernel(P, MFMA), P)
    with pytest.raises(RuntimeError):
        gt.run_wgrad(P, 0, ws_short=1)


def test_vector_pipe_kernels_in_a_child_process():
    """MOPA_CONV2D_MFMA=0 is read once per process: the worker runs every k_conv2d_igemm<...> and k_conv2d_wgrad<...> instantiation
    against float64 (one child process; it prints the worst error per kernel)."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_conv_vector_pipe_worker.py")
    r = subprocess.run([sys.executable, worker], env=dict(os.environ, MOPA_CONV2D_MFMA="0"), timeout=300, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:]
