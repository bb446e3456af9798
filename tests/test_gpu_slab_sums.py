"""The summation order of the split-K weight gradients, bit for bit (the contract of csrc/slabsum.h).

A weight-gradient GEMM leaves one partial result ("slab") per split in the caller's workspace; a second kernel adds the slabs in a
fixed order into the parameter gradient.  Every test here zero-fills the workspace, makes the call, reads the slabs back (as many as
the queried workspace holds: a slab the call did not write is all zero, adds +0 to its lane and changes no bit), redoes the ordered
sum in numpy float32 with explicit loops and compares with the returned gradient by integer view.  Only additions are involved, so
there is no tolerance.

The order: a block of 256 threads takes EW consecutive elements with NL = 256 / EW lanes each.  Lane cl adds slabs cl, cl + NL, ...
in ascending order, starting from +0; then the lanes' sums are added in lane order, either onto the previous gradient
((dw + r0) + r1 + ...: "first") or from +0 with the previous gradient added at the end (dw + (0 + r0 + r1 + ...): "last")."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
needs_mfma = pytest.mark.skipif(os.environ.get("MOPA_CONV2D_MFMA", "1") == "0",
                                reason="the stem's and ConvTranspose2d's one-launch weight gradients are MFMA kernels (MOPA_CONV2D_MFMA=0)")

SENTINEL = 777.0


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def ordered_sum(slabs, nl, prev, assoc):
    """slabs (ns, n) float32, prev (n,) float32 (zeros: a fresh gradient) -> the contract's sum, one float32 addition at a time."""
    ns, n = slabs.shape
    red = np.zeros((nl, n), np.float32)
    for cl in range(nl):                       # lane cl: slabs cl, cl + nl, ... in ascending order, from +0
        for c in range(cl, ns, nl):
            red[cl] = red[cl] + slabs[c]
    t = prev.copy() if assoc == "first" else np.zeros(n, np.float32)
    for k in range(nl):                        # the combine, in lane order
        t = t + red[k]
    out = t if assoc == "first" else prev + t
    assert out.dtype == np.float32
    return out


def read_slabs(ws, n):
    """The (fit, n) slabs a call left in its zero-filled workspace, and how many of them it wrote."""
    fit = ws.numel() // (4 * n)
    slabs = ws[:fit * n * 4].view(torch.float32).reshape(fit, n).cpu().numpy()
    return slabs, int(np.count_nonzero(np.any(slabs != 0, axis=1)))


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def side_of(written, nl, side):
    """The case is on the side of NL it was chosen for: fewer written slabs than lanes, or more and not a multiple."""
    if side == "below":
        assert 0 < written < nl, (written, nl)
    else:
        assert written > nl and written % nl != 0, (written, nl)


# kernel size, channels, EW, H = W of the image, side of NL = 256 / EW the slab count falls on
CONV_CASES = [(1, 64, 16, 24, "below"), (1, 64, 16, 72, "above"),        # n = 4096
              (1, 128, 32, 24, "below"), (1, 128, 32, 72, "above"),      # n = 16384
              (3, 64, 64, 24, "below"), (3, 64, 64, 40, "above")]        # n = 36864


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("k,C,EW,HW,side", CONV_CASES)
def test_conv2d_weight_gradient_is_the_ordered_sum_of_its_slabs(k, C, EW, HW, side, flags):
    """mopa_conv2d_bwd_weight (k_reduce_slabs2<EW>): "first" association; flags bit 1 writes [Cout][Cin][taps]."""
    from mopa_amd._lib import call, ptr, query, stream
    from mopa_amd.dense2d import _geom
    rng = np.random.Generator(np.random.PCG64(1000 * k + C + HW))
    taps, n = k * k, k * k * C * C
    assert EW == (64 if n >= 64 * 512 else 32 if n >= 32 * 512 else 16)
    x, dy = torch.from_numpy(_f32(rng, HW * HW, C)).cuda(), torch.from_numpy(_f32(rng, HW * HW, C)).cuda()
    geom = _geom(B=1, IH=HW, IW=HW, OHl=HW, OWl=HW, OHa=HW, OWa=HW, IY0=-(k // 2), IX0=-(k // 2), TH=k, TW=k, KWF=k, Cin=C, Cout=C,
                 ld_in=C, ld_out=C)
    nbytes = query("mopa_conv2d_wgrad_workspace_bytes", ctypes.addressof(geom))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    prev = _f32(rng, n) if flags & 1 else np.full(n, SENTINEL, np.float32)
    dw = torch.from_numpy(prev).cuda()
    call("mopa_conv2d_bwd_weight", ptr(x), ptr(dy), ptr(dw), ctypes.addressof(geom), flags, ptr(ws), nbytes, stream())
    slabs, written = read_slabs(ws, n)
    side_of(written, 256 // EW, side)
    i = np.arange(n)                                       # i = (tap * Cin + ci) * Cout + co
    o = ((i % C) * C + (i // C) % C) * taps + i // (C * C) if flags & 2 else i
    want = np.empty(n, np.float32)
    want[o] = ordered_sum(slabs, 256 // EW, prev[o] if flags & 1 else np.zeros(n, np.float32), "first")
    same_bits(dw.cpu().numpy(), want, f"{k}x{k} {C}->{C} at {HW}x{HW}, flags {flags}")


@needs_mfma
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("C,EW", [(64, 16), (128, 32)])
def test_convt_weight_gradient_is_the_ordered_sum_of_its_slabs(C, EW, acc):
    """mopa_convt_bwd_weight (k_reduce_slabs_convt<EW>, EW from ONE tap's Cin * Cout elements): "last" association, written into
    ConvTranspose2d's [Cin][Cout][2][2]; 72 x 72 input pixels leave 21 slabs."""
    from mopa_amd._lib import call, ptr, query, stream
    from mopa_amd.dense2d import _geom
    rng = np.random.Generator(np.random.PCG64(2000 + C))
    H = W = 72
    n = 4 * C * C
    assert EW == (64 if C * C >= 64 * 512 else 32 if C * C >= 32 * 512 else 16)
    x, dy = torch.from_numpy(_f32(rng, H * W, C)).cuda(), torch.from_numpy(_f32(rng, 4 * H * W, C)).cuda()
    geom = _geom(B=1, IH=H, IW=W, OHl=H, OWl=W, OHa=2 * H, OWa=2 * W, OS=2, TH=1, TW=1, KWF=2, Cin=C, Cout=C, ld_in=C, ld_out=C)
    nbytes = query("mopa_convt_wgrad_workspace_bytes", ctypes.addressof(geom))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    prev = _f32(rng, n) if acc else np.full(n, SENTINEL, np.float32)
    dw = torch.from_numpy(prev).cuda()
    call("mopa_convt_bwd_weight", ptr(x), ptr(dy), ptr(dw), ctypes.addressof(geom), acc, ptr(ws), nbytes, stream())
    slabs, written = read_slabs(ws, n)
    side_of(written, 256 // EW, "above")
    i = np.arange(n)                                       # i = (tap * Cin + ci) * Cout + co
    o = (((i // C) % C) * C + i % C) * 4 + i // (C * C)
    want = np.empty(n, np.float32)
    want[o] = ordered_sum(slabs, 256 // EW, prev[o] if acc else np.zeros(n, np.float32), "last")
    same_bits(dw.cpu().numpy(), want, f"convT {C}->{C}, accumulate {acc}")


@needs_mfma
@pytest.mark.parametrize("flags", [2, 3])
def test_stem_weight_gradient_is_the_ordered_sum_of_its_slabs(flags):
    """mopa_stem_bwd_weight2 into torch's [64][3][7][7] (k_reduce_slabs_stem: EW = 16, "last" association) on 2 x 97 x 96 output
    pixels: just over 16 x 1,152, so the call leaves 17 slabs.  A slab is [7][2][16][64]: filter row, 4-pixel tap, slot
    4 * (kw % 4) + channel, output channel; the slots of kw = 7 and of the fourth channel are padding and reach no gradient element:
    the 9,408 real ones cover the tensor once, and the floats behind it stay as they were."""
    from mopa_amd._lib import call, ptr, query, stream
    from mopa_amd.dense2d import _geom
    rng = np.random.Generator(np.random.PCG64(3000))
    B, OH, OW, n, nw = 2, 97, 96, 224 * 64, 64 * 3 * 7 * 7
    x4 = torch.from_numpy(_f32(rng, B, OH + 6, OW + 8, 4)).cuda()
    dy = torch.from_numpy(_f32(rng, B * OH * OW, 64)).cuda()
    geom = _geom(B=B, IH=OH + 6, IW=OW + 8, OHl=OH, OWl=OW, OHa=OH, OWa=OW, IDX=4, TH=7, TW=2, KWF=2, Cin=16, Cout=64, ld_in=4, ld_out=64)
    nbytes = query("mopa_conv2d_wgrad_workspace_bytes", ctypes.addressof(geom))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    prev = _f32(rng, nw) if flags & 1 else np.full(nw, SENTINEL, np.float32)
    buf = torch.full((nw + 64,), SENTINEL, device="cuda")
    buf[:nw] = torch.from_numpy(prev).cuda()
    call("mopa_stem_bwd_weight2", ptr(x4), ptr(dy), ptr(buf), ctypes.addressof(geom), flags, ptr(ws), nbytes, stream())
    slabs, written = read_slabs(ws, n)
    side_of(written, 16, "above")
    i = np.arange(n)
    co, k16, tx, kh = i % 64, (i // 64) % 16, (i // 1024) % 2, i // 2048
    kw, c = 4 * tx + k16 // 4, k16 % 4
    live = (kw < 7) & (c < 3)
    p = (((co * 3 + c) * 7 + kh) * 7 + kw)[live]
    assert np.array_equal(np.sort(p), np.arange(nw))
    start = np.zeros(n, np.float32)
    if flags & 1:
        start[live] = prev[p]
    want = np.empty(nw, np.float32)
    want[p] = ordered_sum(slabs, 16, start, "last")[live]
    got = buf.cpu().numpy()
    same_bits(got[:nw], want, f"stem, flags {flags}")
    assert np.all(got[nw:] == SENTINEL)


def _subm_table(rng, rows, size):
    """The 27-offset table [27][rows] of `rows` distinct voxels in a size^3 box: the row of the voxel at each offset, or -1."""
    flat = rng.choice(size ** 3, rows, replace=False)
    xyz = np.stack([flat // (size * size), (flat // size) % size, flat % size], 1)
    row = np.full((size + 2,) * 3, -1, np.int32)
    row[xyz[:, 0] + 1, xyz[:, 1] + 1, xyz[:, 2] + 1] = np.arange(rows, dtype=np.int32)
    offs = [(a, b, c) for a in range(3) for b in range(3) for c in range(3)]
    return np.stack([row[xyz[:, 0] + a, xyz[:, 1] + b, xyz[:, 2] + c] for a, b, c in offs])


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("rows,side", [(600, "below"), (4400, "above")])
def test_sparse_weight_gradient_is_the_ordered_sum_of_its_slabs(rows, side, acc):
    """mopa_spconv_bwd_weight on a 27-offset table, 16 -> 16 channels (k_reduce_slabs: EW = 16, "first" association, identity map):
    3 row chunks and 18."""
    from mopa_amd._lib import call, ptr, query, stream
    rng = np.random.Generator(np.random.PCG64(4000 + rows))
    K, cin, cout = 27, 16, 16
    n = K * cin * cout
    nbr = torch.from_numpy(_subm_table(rng, rows, 12 if rows < 1000 else 20)).cuda()
    x, dout = torch.from_numpy(_f32(rng, rows, cin)).cuda(), torch.from_numpy(_f32(rng, rows, cout)).cuda()
    nbytes = query("mopa_spconv_wgrad_workspace_bytes", K, rows, cin, cout)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    prev = _f32(rng, n) if acc else np.full(n, SENTINEL, np.float32)
    dw = torch.from_numpy(prev).cuda()
    call("mopa_spconv_bwd_weight", ptr(nbr), K, rows, ptr(x), cin, cin, ptr(dout), cout, cout, ptr(dw), acc, ptr(ws), nbytes, stream())
    slabs, written = read_slabs(ws, n)
    side_of(written, 16, side)
    want = ordered_sum(slabs, 16, prev if acc else np.zeros(n, np.float32), "first")
    same_bits(dw.cpu().numpy(), want, f"sparse {rows} rows, accumulate {acc}")
