"""The index map of mopa_amd/csrc/conv2d.hip (ConvGeom) restated in float64, and the table of operator geometries that
tests/test_convgeom_host.py checks it on and tests/test_gpu_conv_tiles.py / tests/_conv_vector_pipe_worker.py run the kernels on.

GEMM view (the comment at the top of conv2d.hip): logical output m = (b, oy, ox) over [B][OHl][OWl] lands at
(oy*OS + OOY, ox*OS + OOX) of [OHa][OWa]; tap (ty, tx) reads input pixel (oy*IS + IY0 + ty*IDY, ox*IS + IX0 + tx*IDX), zero outside
[IH][IW]; its weight slice is w[(KH0 + ty*KS) * KWF + KW0 + tx*KS] of shape [Cin][Cout].

Memory is addressed as the kernels address it: `x` and `out` are FLAT float64 tensors that start at the pointer the entry point
gets (a column slice of a wider buffer starts `col` floats into it), pixel p's channels are x[p * ld_in : p * ld_in + Cin].  That
also covers the stem (Cin = 16 over ld_in = 4: a tap is four consecutive NHWC4 pixels, overlapping its neighbour's), whose expected
value is nevertheless F.conv2d of the 3-channel image with the 7x7 weight (stem_problem).  No HIP here: the geometries come from
mopa_amd.dense2d (ctypes arrays of 25 int32), the rest is torch on the CPU.
"""
from __future__ import annotations

import os
import sys
import zlib
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mopa_amd.dense2d import ConvOp, ConvTOp, Img, _geom  # noqa: E402

FIELDS = ["B", "IH", "IW", "OHl", "OWl", "OHa", "OWa", "OS", "OOY", "OOX", "IS", "IY0", "IX0", "IDY", "IDX",
          "TH", "TW", "KH0", "KW0", "KS", "KWF", "Cin", "Cout", "ld_in", "ld_out"]
DEFECTS = ("tap", "ix0", "last_row", "bias")

# the project's own bounds (tests/test_gpu_2d.py::_close: |got - ref| <= atol * max(1, max|ref|) + rtol * |ref|)
TOL = {"fwd": dict(rtol=1e-4, atol=2e-5), "dgrad": dict(rtol=1e-3, atol=1e-4), "wgrad": dict(rtol=1e-3, atol=1e-4)}


def fields(geom):
    return SimpleNamespace(**{k: int(v) for k, v in zip(FIELDS, geom)})


def _rows(g):
    m = torch.arange(g.B * g.OHl * g.OWl, dtype=torch.int64)
    b, r = m // (g.OHl * g.OWl), m % (g.OHl * g.OWl)
    return b, r // g.OWl, r % g.OWl


def out_index(g):
    """Flat offset of channel 0 of every logical output row m."""
    b, oy, ox = _rows(g)
    return ((b * g.OHa + oy * g.OS + g.OOY) * g.OWa + ox * g.OS + g.OOX) * g.ld_out


def gather(g, x):
    """-> A [M][TH*TW][Cin] (zero where the tap is outside the image), inside [M][TH*TW]."""
    b, oy, ox = _rows(g)
    iy = (oy * g.IS + g.IY0)[:, None] + torch.arange(g.TH) * g.IDY
    ix = (ox * g.IS + g.IX0)[:, None] + torch.arange(g.TW) * g.IDX
    ok = ((iy >= 0) & (iy < g.IH))[:, :, None] & ((ix >= 0) & (ix < g.IW))[:, None, :]
    pix = (b[:, None, None] * g.IH + iy[:, :, None]) * g.IW + ix[:, None, :]
    idx = torch.where(ok, pix * g.ld_in, torch.zeros_like(pix))[..., None] + torch.arange(g.Cin)
    A = x[idx] * ok[..., None]
    return A.reshape(len(b), g.TH * g.TW, g.Cin), ok.reshape(len(b), g.TH * g.TW)


def tap_weights(g, w):
    """w [filter taps][Cin][Cout] -> the logical taps' slices [TH*TW][Cin][Cout]."""
    ty, tx = torch.arange(g.TH)[:, None], torch.arange(g.TW)[None, :]
    return w[((g.KH0 + ty * g.KS) * g.KWF + g.KW0 + tx * g.KS).reshape(-1)]


def _defective(geom, x, defect):
    g = fields(geom)
    if defect == "ix0":
        g.IX0 += 1
    A, ok = gather(g, x)
    if defect == "tap":   # the last in-image (row, tap) pair that holds data (the stem's frame is zero padding) reads zero
        m, t = [int(v[-1]) for v in torch.nonzero(ok & (A.abs().sum(-1) > 0), as_tuple=True)]
        A[m, t] = 0
    rows = len(A) - 1 if defect == "last_row" else len(A)
    return g, A, rows


def igemm_ref(geom, x, w, bias, out, accumulate, defect=None):
    """What mopa_conv2d_igemm leaves in `out` (a new tensor; elements outside the logical grid keep their value).
    defect: one of DEFECTS -- a deliberately wrong restatement, for the sensitivity test."""
    assert defect is None or defect in DEFECTS
    g, A, rows = _defective(geom, x, defect)
    res = torch.einsum("mtc,tcn->mn", A, tap_weights(g, w))
    if bias is not None and defect != "bias":
        res = res + bias
    idx = out_index(g)[:rows, None] + torch.arange(g.Cout)
    out = out.clone()
    out[idx] = res[:rows] + (out[idx] if accumulate else 0)
    return out


def touched(geom, n):
    """bool [n]: the elements of the flat output that the launch writes."""
    g = fields(geom)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[out_index(g)[:, None] + torch.arange(g.Cout)] = True
    return mask


def wgrad_ref(geom, x, dy, defect=None):
    """dW[tap][ci][co] = sum_m A[m][tap][ci] * dY[m][co]: mopa_conv2d_bwd_weight's tap-major layout."""
    assert defect in (None, "tap", "ix0", "last_row")
    g, A, rows = _defective(geom, x, defect)
    dY = dy[out_index(g)[:, None] + torch.arange(g.Cout)]
    return torch.einsum("mtc,mn->tcn", A[:rows], dY[:rows])


def oihw(dw):
    """[tap][ci][co] -> torch's parameter layout [co][ci][tap] (flags bit 1 of mopa_conv2d_bwd_weight)."""
    return dw.permute(2, 1, 0).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# Problems: data in the buffers the kernels see, and what torch says the operator computes
IN_SENTINEL, OUT_SENTINEL = 1.0e6, -77.0


def _rng(name):
    return np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))


def _randn(rng, *shape, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * np.float32(scale))


def _rows_of(t):   # NCHW -> [B*H*W][C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _wide(rows, C, pad_left, pad_right, fill, dense=None):
    """[rows][pad_left + C + pad_right] filled with `fill`, `dense` ([rows][C]) in its middle columns."""
    t = torch.full((rows, pad_left + C + pad_right), fill, dtype=torch.float32)
    if dense is not None:
        t[:, pad_left:pad_left + C] = dense
    return t


def flat(wide, col):
    """The float64 memory behind the pointer of column `col` of a wide buffer."""
    return wide.double().reshape(-1)[col:]


def _problem(name, role, geoms, xw, xcol, w, bias, out_shape, ocol, expect, **more):
    """xw / xcol: the input's wide buffer and column; w: [filter taps][Cin][Cout]; out_shape / ocol: the output's wide buffer and
    column; expect: torch's float64 result as dense rows [pixels][Cout]."""
    return SimpleNamespace(name=name, role=role, geoms=geoms, xw=xw, xcol=xcol, w=w, bias=bias, out_shape=out_shape, ocol=ocol,
                           expect=expect, **more)


# kind -> (k, s, p); grid = (B, OHl, OWl): the logical grid of the launch (of the first and largest class where there are four)
CONVS = {"conv3s1": (3, 1, 1), "conv3s2": (3, 2, 1), "conv1s2": (1, 2, 0)}
DGRADS = {"dgrad3s1": (3, 1, 1), "dgrad3s2": (3, 2, 1), "dgrad1s2": (1, 2, 0)}
KINDS = list(CONVS) + list(DGRADS) + ["convt", "convt_bwd", "wino", "stem"]
# M = 1 (1x1 image), 2 (2x1 image), 63, 64, 65, 129, 255, 256, 257 (one image row), 270; B = 3: tiles cross image borders
GRIDS = [(1, 1, 1), (1, 2, 1), (3, 3, 7), (1, 8, 8), (1, 5, 13), (1, 3, 43), (3, 5, 17), (1, 16, 16), (1, 1, 257), (3, 9, 10)]
CHANNELS = [(16, 64), (48, 128), (64, 64), (16, 128), (48, 64), (64, 128)]   # (Cin, Cout) of the GEMM: 1, 3, 4 chunks x 64, 128
# weight-gradient pixel counts 1, 15, 16, 17, 257, 513: shorter than / exactly / just over one 16-pixel stage, 2 and 3 slices
WGRAD_GRIDS = [(1, 1, 1), (1, 3, 5), (2, 2, 4), (1, 1, 17), (1, 1, 257), (3, 9, 19)]
# the stem's one-block MFMA kernel takes 1152 pixels per slice: 1260 and 2349 pixels are its 2 and 3 slices, the last partly filled
STEM_WGRAD_GRIDS = WGRAD_GRIDS + [(3, 20, 21), (3, 29, 27)]


def _in_hw(k, s, oh, ow, even=False):
    """An input size whose convolution (k, s, p = k // 2) has the output grid oh x ow (stride 2: the odd one unless `even`)."""
    if s == 1:
        return oh, ow
    return (2 * oh, 2 * ow) if even else (2 * oh - 1, 2 * ow - 1)


def conv_problem(kind, grid, cin, cout, bias, name=None):
    """Forward Conv2d (ConvOp._fwd_geom); also the weight-gradient problem of the same layer (dy, dw_expect)."""
    k, s, p = CONVS[kind]
    B, oh, ow = grid
    H, W = _in_hw(k, s, oh, ow, even=(k == 1))
    name = name or f"{kind}-{B}x{oh}x{ow}-{cin}-{cout}"
    rng = _rng(name)
    x = _randn(rng, B, cin, H, W)
    w = _randn(rng, cout, cin, k, k, scale=0.05)
    b = _randn(rng, cout) if bias else None
    gout = _randn(rng, B, cout, oh, ow)
    wd = w.double().requires_grad_(True)
    ref = F.conv2d(x.double(), wd, None if b is None else b.double(), s, p)
    assert tuple(ref.shape) == (B, cout, oh, ow)
    (ref * gout.double()).sum().backward()
    xw = _wide(B * H * W, cin, 4, 8, IN_SENTINEL, _rows_of(x))
    dyw = _wide(B * oh * ow, cout, 8, 4, IN_SENTINEL, _rows_of(gout))
    op = ConvOp(w, b, k, s, p)
    geom = op._fwd_geom(Img(xw, B, H, W, 4, cin), Img(dyw, B, oh, ow, 8, cout))
    return _problem(name, "fwd", [geom], xw, 4, w.permute(2, 3, 1, 0).reshape(k * k, cin, cout).contiguous(), b,
                    tuple(dyw.shape), 8, _rows_of(ref.detach()), dyw=dyw, dw_expect=wd.grad.permute(2, 3, 1, 0).reshape(k * k, cin, cout))


def dgrad_problem(kind, grid, cin, cout, name=None):
    """Backward-data of Conv2d: the GEMM reads the output gradient (Cin channels of it) and writes dx (Cout channels).
    Stride 1: the geometry of ConvOp.backward; stride 2: the classes of ConvOp.dgrad_s2_geoms, grid = class (0, 0)."""
    k, s, p = DGRADS[kind]
    B, oh, ow = grid
    H, W = _in_hw(k, s, oh, ow)            # dx is H x W; its class (0, 0) (or all of it) is the grid
    dh, dw_ = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    name = name or f"{kind}-{B}x{oh}x{ow}-{cin}-{cout}"
    rng = _rng(name)
    O, I = cin, cout
    w = _randn(rng, O, I, k, k, scale=0.05)
    gout = _randn(rng, B, O, dh, dw_)
    xr = torch.zeros(B, I, H, W, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xr, w.double(), None, s, p) * gout.double()).sum().backward()
    gw = _wide(B * dh * dw_, O, 8, 4, IN_SENTINEL, _rows_of(gout))
    dxw = _wide(B * H * W, I, 4, 12, OUT_SENTINEL)
    op = ConvOp(w, None, k, s, p)
    xi, di, dxi = Img(dxw, B, H, W, 4, I), Img(gw, B, dh, dw_, 8, O), Img(dxw, B, H, W, 4, I)
    if s == 1:   # (ConvOp.backward)
        geoms = [_geom(B=B, IH=dh, IW=dw_, OHl=H, OWl=W, OHa=H, OWa=W, IY0=p, IX0=p, IDY=-1, IDX=-1, TH=k, TW=k, KWF=k, Cin=O,
                       Cout=I, ld_in=di.ld, ld_out=dxi.ld)]
    else:
        geoms = op.dgrad_s2_geoms(xi, di, dxi)
        g0 = fields(geoms[0])
        assert (g0.OHl, g0.OWl) == (oh, ow)
    return _problem(name, "dgrad", geoms, gw, 8, w.permute(2, 3, 0, 1).reshape(k * k, O, I).contiguous(), None, tuple(dxw.shape), 4,
                    _rows_of(xr.grad))


def convt_problem(kind, grid, cin, cout, bias, name=None):
    """ConvTranspose2d(k2, s2): the four classes of ConvTOp._geom, or (convt_bwd) its backward-data, the 2x2 stride-2 convolution of
    ConvTOp.backward (the GEMM reads Cin channels of the output gradient and writes Cout channels of dx)."""
    B, H, W = grid
    name = name or f"{kind}-{B}x{H}x{W}-{cin}-{cout}"
    rng = _rng(name)
    if kind == "convt":
        x = _randn(rng, B, cin, H, W)
        w = _randn(rng, cin, cout, 2, 2, scale=0.05)
        b = _randn(rng, cout) if bias else None
        ref = F.conv_transpose2d(x.double(), w.double(), None if b is None else b.double(), 2)
        xw = _wide(B * H * W, cin, 4, 8, IN_SENTINEL, _rows_of(x))
        ow_ = _wide(B * 4 * H * W, cout, 8, 4, OUT_SENTINEL)
        op = ConvTOp(w, b)
        xi, oi = Img(xw, B, H, W, 4, cin), Img(ow_, B, 2 * H, 2 * W, 8, cout)
        geoms = [op._geom(xi, oi, ky, kx) for ky in range(2) for kx in range(2)]
        return _problem(name, "fwd", geoms, xw, 4, w.permute(2, 3, 0, 1).reshape(4, cin, cout).contiguous(), b, tuple(ow_.shape), 8,
                        _rows_of(ref))
    I, O = cout, cin
    w = _randn(rng, I, O, 2, 2, scale=0.05)
    gout = _randn(rng, B, O, 2 * H, 2 * W)
    xr = torch.zeros(B, I, H, W, dtype=torch.float64, requires_grad=True)
    (F.conv_transpose2d(xr, w.double(), None, 2) * gout.double()).sum().backward()
    gw = _wide(B * 4 * H * W, O, 8, 4, IN_SENTINEL, _rows_of(gout))
    dxw = _wide(B * H * W, I, 4, 12, OUT_SENTINEL)
    geom = _geom(B=B, IH=2 * H, IW=2 * W, OHl=H, OWl=W, OHa=H, OWa=W, IS=2, TH=2, TW=2, KWF=2, Cin=O, Cout=I, ld_in=gw.shape[1],
                 ld_out=dxw.shape[1])
    return _problem(name, "dgrad", [geom], gw, 8, w.permute(2, 3, 1, 0).reshape(4, O, I).contiguous(), None, tuple(dxw.shape), 4,
                    _rows_of(xr.grad))


def wino_geom(T, cin, cout, ld_in=None, ld_out=None):
    """The flat geometry that wino_conv hands to mopa_conv2d_igemm_batched: T rows of one 1x1 problem."""
    return _geom(B=1, IH=1, IW=T, OHl=1, OWl=T, OHa=1, OWa=T, TH=1, TW=1, KWF=1, Cin=cin, Cout=cout, ld_in=ld_in or cin,
                 ld_out=ld_out or cout)


def wino_problem(grid, cin, cout, name=None):
    T = grid[0] * grid[1] * grid[2]
    name = name or f"wino-{T}-{cin}-{cout}"
    rng = _rng(name)
    x, w = _randn(rng, T, cin), _randn(rng, cin, cout, scale=0.05)
    xw, ow_ = _wide(T, cin, 4, 8, IN_SENTINEL, x), _wide(T, cout, 8, 4, OUT_SENTINEL)
    return _problem(name, "fwd", [wino_geom(T, cin, cout, xw.shape[1], ow_.shape[1])], xw, 4, w.reshape(1, cin, cout), None,
                    tuple(ow_.shape), 8, x.double() @ w.double())


def img_to_nhwc4(img, Hp, Wp):
    """mopa_img_to_nhwc4: NCHW (B, 3, H, W) -> zero-padded NHWC4 (B, Hp + 6, Wp + 8, 4), the image at (3, 3), channel 3 zero."""
    B, _, H, W = img.shape
    out = torch.zeros(B, Hp + 6, Wp + 8, 4, dtype=img.dtype)
    out[:, 3:3 + H, 3:3 + W, :3] = img.permute(0, 2, 3, 1)
    return out


def stem_relayout(w):
    """mopa_conv2d_stem_relayout: OIHW (O, 3, 7, 7) -> [7][2][16][O]; tap (kh, tx) slot k16 is kw = 4 tx + k16 // 4, c = k16 % 4."""
    O = w.shape[0]
    full = torch.zeros(O, 4, 7, 8, dtype=w.dtype)
    full[:, :3, :, :7] = w
    return full.permute(2, 3, 1, 0).reshape(7, 2, 4, 4, O).reshape(7, 2, 16, O).contiguous()


def stem_problem(grid, pad=(0, 0), name=None):
    """The 7x7 stem through the 16-wide tap trick (Cin = 16 over ld_in = 4, IDX = 4, 7 x 2 taps) as mopa_amd.dense2d launches it;
    grid = (B, Hp, Wp), the image is pad smaller.  Expected: F.conv2d of the 3-channel image in the padded frame, 7x7, padding 3."""
    B, Hp, Wp = grid
    H, W = Hp - pad[0], Wp - pad[1]
    name = name or f"stem-{B}x{Hp}x{Wp}"
    rng = _rng(name)
    img = _randn(rng, B, 3, H, W)
    w = _randn(rng, 64, 3, 7, 7, scale=0.05)
    gout = _randn(rng, B, 64, Hp, Wp)
    wd = w.double().requires_grad_(True)
    framed = F.pad(img.double(), (0, Wp - W, 0, Hp - H))
    ref = F.conv2d(framed, wd, None, 1, 3)
    (ref * gout.double()).sum().backward()
    x4 = img_to_nhwc4(img, Hp, Wp)
    ow_ = _wide(B * Hp * Wp, 64, 64, 0, IN_SENTINEL, _rows_of(gout))    # the right half of a join buffer
    geom = _geom(B=B, IH=Hp + 6, IW=Wp + 8, OHl=Hp, OWl=Wp, OHa=Hp, OWa=Wp, IDX=4, TH=7, TW=2, KWF=2, Cin=16, Cout=64, ld_in=4,
                 ld_out=ow_.shape[1])
    # the weight gradient in the kernel's layout: the real slots are the parameter's, the others (kw = 7: the pixel right of the
    # window; c = 3: the zero channel) are whatever the index map says -- wgrad_ref is their only statement
    return _problem(name, "fwd", [geom], x4.reshape(-1, 4), 0, stem_relayout(w).reshape(14, 16, 64), None, tuple(ow_.shape), 64,
                    _rows_of(ref.detach()), dyw=ow_, dw_expect=stem_relayout(wd.grad).reshape(14, 16, 64),
                    dw_real=stem_relayout(torch.ones(64, 3, 7, 7)).reshape(14, 16, 64) > 0, img=img, w_oihw=w)


def problem(kind, grid, cin=64, cout=64, bias=False):
    if kind in CONVS:
        return conv_problem(kind, grid, cin, cout, bias)
    if kind in DGRADS:
        return dgrad_problem(kind, grid, cin, cout)
    if kind in ("convt", "convt_bwd"):
        return convt_problem(kind, grid, cin, cout, bias)
    if kind == "wino":
        return wino_problem(grid, cin, cout)
    assert kind == "stem"
    return stem_problem(grid, pad=(1, 2) if grid[1] > 2 and grid[2] > 2 else (0, 0))


def igemm_cases():
    """(kind, grid, Cin, Cout, bias) of every operator geometry at every grid.  The channel pair rotates with ki + gi (odd: 128 output
    channels), the bias with (ki + gi) // 2, so that a bias meets 64 and 128 output channels (more than one column tile, the
    128-wide tile) and so does NULL."""
    out = []
    for ki, kind in enumerate(KINDS):
        for gi, grid in enumerate(GRIDS):
            cin, cout = (16, 64) if kind == "stem" else CHANNELS[(ki + gi) % len(CHANNELS)]
            out.append((kind, grid, cin, cout, (kind in CONVS or kind == "convt") and (ki + gi) // 2 % 2 == 0))
    return out


def wgrad_cases():
    """(kind, grid, Cin, Cout): 3x3 s1, 3x3 s2, 1x1 s2 at Cin = 64 (the MFMA kernels <3,1>, <1,1>; vector <64,3>, <64,1>) and Cin = 16
    (vector <16,1>), and the stem (k_stem_wgrad_mfma; vector <16,2>)."""
    out = []
    for ki, kind in enumerate(CONVS):
        for gi, grid in enumerate(WGRAD_GRIDS):
            for cin in (64, 16):
                out.append((kind, grid, cin, (64, 128)[(ki + gi) % 2]))
    return out + [("stem", grid, 16, 64) for grid in STEM_WGRAD_GRIDS]


def case_id(case):
    kind, (B, h, w), cin, cout = case[:4]
    return f"{kind}-{B}x{h}x{w}-{cin}-{cout}"


def bound(ref, role):
    """The elementwise bound of tests/test_gpu_2d.py::_close for a float64 reference tensor."""
    t = TOL[role]
    return t["atol"] * max(1.0, float(ref.abs().max())) + t["rtol"] * ref.abs()
