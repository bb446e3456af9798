"""Launch and comparison helpers of tests/test_gpu_conv_tiles.py and tests/_conv_vector_pipe_worker.py: the problems of
tests/_convgeom_reference.py on the GPU through mopa_conv2d_igemm, mopa_conv2d_igemm_classes and mopa_conv2d_bwd_weight, compared with
the float64 restatement under the bounds of tests/test_gpu_2d.py::_close, and the worst error seen per kernel."""
import ctypes
import sys
import zlib
from types import SimpleNamespace

import numpy as np
import torch

import _convgeom_reference as cr
from mopa_amd._lib import call, host_i32, ptr, query, stream

TILES = ("256x64", "128x128", "128x64", "64x64")   # kTiles of conv2d.hip; flags bits 8-15 = index + 1
WORST = {}   # kernel -> [largest error / bound, largest |error| / max|ref|]


def note(kernel, err, bound, ref):
    """Record one comparison; -> the fraction of the bound it used."""
    used = float((err / bound).max())
    rel = float(err.max()) / max(float(ref.abs().max()), 1e-30)
    w = WORST.setdefault(kernel, [0.0, 0.0])
    w[0], w[1] = max(w[0], used), max(w[1], rel)
    return used


def report(out=sys.stdout):
    for k in sorted(WORST):
        print(f"[conv tiles] {k}: worst error {WORST[k][0]:.3f} of its bound, {WORST[k][1]:.2e} of max|ref|", file=out, flush=True)


def tile_flags(tile):
    return 0 if tile is None else (tile + 1) << 8


def device(P):
    """The problem's inputs on the GPU (once).  The stem's go through mopa_img_to_nhwc4 and mopa_conv2d_stem_relayout, as
    mopa_amd.dense2d prepares them, and must be what the table holds."""
    if not hasattr(P, "dev"):
        d = SimpleNamespace(x=P.xw.cuda(), w=P.w.cuda(), b=None if P.bias is None else P.bias.cuda(),
                            dy=P.dyw.cuda() if hasattr(P, "dyw") else None)
        if hasattr(P, "img"):
            B, _, H, W = P.img.shape
            g = cr.fields(P.geoms[0])
            img, w = P.img.cuda(), P.w_oihw.cuda()
            x4 = torch.full((B, g.IH, g.IW, 4), 9.0, device="cuda")
            w1 = torch.full((7, 2, 16, 64), 9.0, device="cuda")
            call("mopa_img_to_nhwc4", ptr(img), B, H, W, g.OHl, g.OWl, ptr(x4), stream())
            call("mopa_conv2d_stem_relayout", ptr(w), ptr(w1), 64, 0, 0, stream())
            assert torch.equal(x4.cpu().reshape(-1, 4), P.xw) and torch.equal(w1.cpu().reshape(14, 16, 64), P.w)
            d.x, d.w = x4.reshape(-1, 4), w1.reshape(14, 16, 64)
        P.dev = d
    return P.dev


def initial_out(P, accumulate):
    """The output buffer before the launch: the sentinel everywhere, or (accumulate) random previous values everywhere."""
    if not accumulate:
        return torch.full(P.out_shape, cr.OUT_SENTINEL, dtype=torch.float32)
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(("previous " + P.name).encode())))
    return torch.from_numpy(rng.standard_normal(P.out_shape).astype(np.float32))


def igemm_expect(P, init, accumulate):
    """-> (the float64 flat output after every class of the problem, the mask of the elements they write)."""
    x, w = cr.flat(P.xw, P.xcol), P.w.double()
    bias = None if P.bias is None else P.bias.double()
    out = cr.flat(init, P.ocol)
    mask = torch.zeros(len(out), dtype=torch.bool)
    for g in P.geoms:
        out = cr.igemm_ref(g, x, w, bias, out, accumulate)
        mask |= cr.touched(g, len(out))
    if hasattr(P, "img"):   # the stem's reference is F.conv2d of the 3-channel image itself
        wide = init.double()
        cols = slice(P.ocol, P.ocol + P.expect.shape[1])
        wide[:, cols] = P.expect + (wide[:, cols] if accumulate else 0)
        assert float((wide.reshape(-1)[P.ocol:] - out).abs().max()) <= 1e-9
        out = wide.reshape(-1)[P.ocol:]
    return out, mask


def run_igemm(P, tile, accumulate, init, classes=False, geoms=None):
    """One mopa_conv2d_igemm per class (or one mopa_conv2d_igemm_classes) into a copy of `init`; -> the whole wide buffer."""
    d = device(P)
    out = init.cuda()
    flags = int(accumulate) | tile_flags(tile)
    geoms = P.geoms if geoms is None else geoms
    if classes:
        g4 = host_i32([v for g in geoms for v in g])
        call("mopa_conv2d_igemm_classes", ptr(d.x, P.xcol), ptr(d.w), ptr(d.b), ptr(out, P.ocol), ctypes.addressof(g4), flags, stream())
    else:
        for g in geoms:
            call("mopa_conv2d_igemm", ptr(d.x, P.xcol), ptr(d.w), ptr(d.b), ptr(out, P.ocol), ctypes.addressof(g), flags, stream())
    return out.cpu()


def check_igemm(kernel, P, got, init, ref, mask):
    """Outside `mask` (sentinel columns, pixels of other parity classes) the buffer is untouched; inside, float64 within the bound."""
    full = torch.zeros(got.numel(), dtype=torch.bool)
    full[P.ocol:] = mask
    assert torch.equal(got.reshape(-1)[~full], init.reshape(-1)[~full]), f"{P.name}: wrote outside its elements"
    g, r = got.double().reshape(-1)[full], ref[mask]
    assert bool(torch.isfinite(g).all()), f"{P.name}: non-finite output"
    used = note(kernel, (g - r).abs(), cr.bound(r, P.role), r)
    assert used <= 1.0, f"{P.name} {kernel}: error {used:.2f} x the bound"


def wgrad_kernel(P, mfma):
    g = cr.fields(P.geoms[0])
    if g.Cin >= 64:
        return ("k_conv2d_wgrad_mfma<%d,1>" if mfma else "k_conv2d_wgrad<64,%d>") % (3 if g.TW % 3 == 0 else 1)
    if g.TW == 2:
        return "k_stem_wgrad_mfma" if mfma and g.TH == 7 and g.Cout == 64 else "k_conv2d_wgrad<16,2>"
    return "k_conv2d_wgrad<16,1>"


def run_wgrad(P, flags, prev=None, ws_short=0):
    """mopa_conv2d_bwd_weight into a [taps][Cin][Cout] (or, flags bit 1, [Cout][Cin][taps]) tensor; prev: its previous content."""
    d = device(P)
    g = cr.fields(P.geoms[0])
    shape = (g.Cout, g.Cin, g.TH * g.TW) if flags & 2 else (g.TH * g.TW, g.Cin, g.Cout)
    dw = torch.full(shape, cr.OUT_SENTINEL, device="cuda") if prev is None else prev.cuda()
    nbytes = query("mopa_conv2d_wgrad_workspace_bytes", ctypes.addressof(P.geoms[0]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    call("mopa_conv2d_bwd_weight", ptr(d.x, P.xcol), ptr(d.dy, P.ocol), ptr(dw), ctypes.addressof(P.geoms[0]), flags, ptr(ws),
         nbytes - ws_short, stream())
    return dw.cpu()


def check_wgrad(kernel, P):
    """Both layouts, fresh and accumulated onto a previous value, against wgrad_ref; two runs give the same bits."""
    ref = cr.wgrad_ref(P.geoms[0], cr.flat(P.xw, P.xcol), cr.flat(P.dyw, P.ocol))
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(("previous dw " + P.name).encode())))
    for layout in (0, 2):
        want = cr.oihw(ref) if layout else ref
        got = run_wgrad(P, layout)
        assert torch.equal(got, run_wgrad(P, layout)), f"{P.name}: two runs differ"
        prev = torch.from_numpy(rng.standard_normal(tuple(want.shape)).astype(np.float32))
        acc = run_wgrad(P, layout | 1, prev)
        for name, g, r in (("fresh", got, want), ("accumulated", acc, want + prev.double())):
            assert bool(torch.isfinite(g).all()), f"{P.name}: non-finite {name} gradient"
            used = note(kernel, (g.double() - r).abs(), cr.bound(r, "wgrad"), r)
            assert used <= 1.0, f"{P.name} {kernel} layout {layout} {name}: error {used:.2f} x the bound"
