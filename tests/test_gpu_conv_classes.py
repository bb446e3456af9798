"""The four parity classes of ConvTranspose2d(k2, s2) (forward, weight gradient) and of a stride-2 convolution's backward-data in ONE
launch (dense2d.CONV_CLASSES: mopa_conv2d_igemm_classes, mopa_convt_bwd_weight) against one launch per class: identical bits, and both
against the fp64 torch reference with the tolerances of tests/test_gpu_2d.py::test_conv_transpose_fwd_bwd."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _nhwc(t):  # (B,C,H,W) cpu -> Img on cuda
    from mopa_amd.dense2d import Img
    B, C, H, W = t.shape
    return Img(t.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous().cuda(), B, H, W)


def _nchw(img):
    return img.dense().reshape(img.B, img.H, img.W, img.C).permute(0, 3, 1, 2).cpu()


def _close(got, ref, rtol=1e-4, atol=2e-5):   # (tests/test_gpu_2d.py::_close)
    ref = ref.detach().float().numpy() if torch.is_tensor(ref) else ref
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol * max(1.0, float(np.abs(ref).max())))


def _logged(monkeypatch, dense2d):
    calls = []
    inner = dense2d.call
    monkeypatch.setattr(dense2d, "call", lambda name, *a: (calls.append(name), inner(name, *a))[1])
    return calls


def _right_half(B, H, W, C, fill):
    """An image in the right half of a buffer twice as wide, every element pre-filled."""
    from mopa_amd.dense2d import Img
    wide = torch.full((B * H * W, 2 * C), fill, dtype=torch.float32, device="cuda")
    return wide, Img(wide, B, H, W, C, C)


# M = B H W input pixels: 30 (less than one tile), 126 (a ragged second tile), 405, 960 (four K-splits that straddle image rows)
CONVT_SHAPES = [(2, 64, 64, 3, 5), (2, 128, 64, 7, 9), (3, 64, 128, 9, 15), (2, 64, 64, 20, 24)]


def _convt_run(monkeypatch, on, B, cin, cout, H, W, x, w, b, gout, dw0):
    from mopa_amd import dense2d
    monkeypatch.setattr(dense2d, "CONV_CLASSES", on)
    calls = _logged(monkeypatch, dense2d)
    op = dense2d.ConvTOp(w.cuda(), b.cuda())
    xi = _nhwc(x)
    wide, out = _right_half(B, 2 * H, 2 * W, cout, 7.0)
    op.forward(xi, out)
    # the output gradient, too, lives in the right half of a wider buffer
    gwide, gi = _right_half(B, 2 * H, 2 * W, cout, 3.0)
    gwide[:, cout:] = _nhwc(gout).t
    dx = dense2d.new_img(B, H, W, cin, "cuda")
    dw, db = torch.empty_like(op.w), torch.empty_like(op.b)
    op.backward(xi, gi, dx, dw, db)                        # written
    dwa, dba = dw0.cuda().clone(), torch.ones_like(op.b)
    op.backward(xi, gi, dx, dwa, dba, acc_params=True)     # accumulated
    torch.cuda.synchronize()
    return dict(wide=wide, out=_nchw(out), dx=_nchw(dx), dw=dw.cpu(), db=db.cpu(), dwa=dwa.cpu()), list(calls)


@pytest.mark.parametrize("B,cin,cout,H,W", CONVT_SHAPES)
def test_conv_transpose_one_launch_per_pass(B, cin, cout, H, W, monkeypatch):
    rng = np.random.Generator(np.random.PCG64(cin + cout + H))
    x = torch.from_numpy(rng.standard_normal((B, cin, H, W), dtype=np.float32))
    w = torch.from_numpy(rng.standard_normal((cin, cout, 2, 2), dtype=np.float32) * 0.05)
    b = torch.from_numpy(rng.standard_normal(cout, dtype=np.float32))
    dw0 = torch.from_numpy(rng.standard_normal((cin, cout, 2, 2), dtype=np.float32))
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.conv_transpose2d(xr, wr, br, 2)
    gout = torch.from_numpy(rng.standard_normal(tuple(ref.shape), dtype=np.float32))
    (ref * gout.double()).sum().backward()
    old, c_old = _convt_run(monkeypatch, False, B, cin, cout, H, W, x, w, b, gout, dw0)
    new, c_new = _convt_run(monkeypatch, True, B, cin, cout, H, W, x, w, b, gout, dw0)
    # today's launches with the switch off; with it on, one launch forward and one entry point per weight gradient, no re-layout
    assert "mopa_conv2d_igemm_classes" not in c_old and "mopa_convt_bwd_weight" not in c_old
    assert c_old.count("mopa_conv2d_bwd_weight") == 8 and c_old.count("mopa_conv2d_igemm") == 4 + 2
    assert c_new.count("mopa_conv2d_igemm_classes") == 1 and c_new.count("mopa_convt_bwd_weight") == 2
    assert c_new.count("mopa_conv2d_igemm") == 2   # (the two backward-data calls)
    assert "mopa_conv2d_bwd_weight" not in c_new
    for k in old:
        assert torch.equal(old[k], new[k]), (k, float((old[k] - new[k]).abs().max()))
    assert bool((new["wide"][:, :cout] == 7.0).all())       # the left half of the join buffer is untouched
    _close(new["out"], ref)
    _close(new["dx"], xr.grad, rtol=1e-3, atol=1e-4)
    _close(new["dw"], wr.grad, rtol=1e-3, atol=1e-4)
    _close(new["db"], br.grad, rtol=1e-3, atol=1e-4)
    _close(new["dwa"] - dw0, wr.grad, rtol=1e-3, atol=1e-4)


def _dgrad_run(monkeypatch, on, k, p, B, cin, cout, H, W, x, w, gout):
    from mopa_amd import dense2d
    monkeypatch.setattr(dense2d, "CONV_CLASSES", on)
    calls = _logged(monkeypatch, dense2d)
    op = dense2d.ConvOp(w.cuda(), None, k, 2, p)
    xi, gi = _nhwc(x), _nhwc(gout)
    dw = torch.empty_like(op.w)
    wide_a, dxa = _right_half(B, H, W, cin, 1.0)    # a reader's share is there already: accumulate
    op.backward(xi, gi, dxa, dw, None, acc_dx=True)
    wide_w, dxw = _right_half(B, H, W, cin, 5.0)    # first writer: whatever the buffer held is replaced
    op.backward(xi, gi, dxw, dw, None, acc_dx=False)
    torch.cuda.synchronize()
    return dict(wide_a=wide_a, wide_w=wide_w, dxa=_nchw(dxa), dxw=_nchw(dxw)), list(calls)


@pytest.mark.parametrize("k,p,H,W", [(3, 1, 7, 9),     # four classes of different sizes (4x5, 4x4, 3x5, 3x4 pixels per image)
                                      (3, 1, 8, 10),
                                      (1, 0, 7, 9)])    # the 1x1 downsample: one non-empty class, the per-class path stays
def test_stride2_backward_data_one_launch(k, p, H, W, monkeypatch):
    B, cin, cout = 2, 64, 128   # 128 output-gradient channels -> 64
    rng = np.random.Generator(np.random.PCG64(k + H))
    x = torch.from_numpy(rng.standard_normal((B, cin, H, W), dtype=np.float32))
    w = torch.from_numpy(rng.standard_normal((cout, cin, k, k), dtype=np.float32) * 0.05)
    xr = x.double().requires_grad_(True)
    ref = F.conv2d(xr, w.double(), None, 2, p)
    gout = torch.from_numpy(rng.standard_normal(tuple(ref.shape), dtype=np.float32))
    (ref * gout.double()).sum().backward()
    old, c_old = _dgrad_run(monkeypatch, False, k, p, B, cin, cout, H, W, x, w, gout)
    new, c_new = _dgrad_run(monkeypatch, True, k, p, B, cin, cout, H, W, x, w, gout)
    assert "mopa_conv2d_igemm_classes" not in c_old
    if k == 3:
        assert (c_old.count("mopa_conv2d_igemm"), c_old.count("mopa_zero_rows")) == (8, 1)
        assert (c_new.count("mopa_conv2d_igemm_classes"), c_new.count("mopa_conv2d_igemm"), c_new.count("mopa_zero_rows")) == (2, 0, 0)
    else:
        assert c_new == c_old and (c_new.count("mopa_conv2d_igemm"), c_new.count("mopa_zero_rows")) == (2, 1)
        assert bool((new["dxw"][:, :, 1::2] == 0).all()) and bool((new["dxw"][:, :, :, 1::2] == 0).all())   # the empty classes
    for key in old:
        assert torch.equal(old[key], new[key]), (key, float((old[key] - new[key]).abs().max()))
    assert bool((new["wide_a"][:, :cin] == 1.0).all()) and bool((new["wide_w"][:, :cin] == 5.0).all())
    _close(new["dxw"], xr.grad, rtol=1e-3, atol=1e-4)
    _close(new["dxa"] - 1.0, xr.grad, rtol=1e-3, atol=1e-4)


def test_classes_tile_does_not_change_the_bits():
    """The one-launch form chooses its tile from the rows of all four classes (128 x 64 where a class alone would take 64 x 64): every
    output element sees the same channel chunks and MFMA sequence under either tile."""
    from mopa_amd._lib import call, host_i32, ptr, stream
    from mopa_amd.dense2d import ConvTOp, new_img, relayout_cached
    rng = np.random.Generator(np.random.PCG64(11))
    B, cin, cout, H, W = 2, 128, 64, 9, 11
    x = _nhwc(torch.from_numpy(rng.standard_normal((B, cin, H, W), dtype=np.float32)))
    op = ConvTOp(torch.from_numpy(rng.standard_normal((cin, cout, 2, 2), dtype=np.float32)).cuda(),
                 torch.from_numpy(rng.standard_normal(cout, dtype=np.float32)).cuda())
    wl = relayout_cached(op.w, (2, 2, cin, cout), cout, cin, 2, 2, 2)
    outs = []
    for tile in (3, 2):   # kTiles: 64 x 64, 128 x 64
        out = new_img(B, 2 * H, 2 * W, cout, "cuda")
        g4 = host_i32([v for ky in range(2) for kx in range(2) for v in op._geom(x, out, ky, kx)])
        call("mopa_conv2d_igemm_classes", x.p, ptr(wl), ptr(op.b), out.p, ctypes.addressof(g4), (tile + 1) << 8, stream())
        outs.append(out.t)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])


def test_entry_points_refuse_what_they_cannot_run():
    from mopa_amd._lib import call, host_i32, ptr, query, stream, workspace
    from mopa_amd.dense2d import ConvTOp, new_img
    B, cin, cout, H, W = 2, 64, 64, 3, 5
    x = new_img(B, H, W, cin, "cuda", zero=True)
    out = new_img(B, 2 * H, 2 * W, cout, "cuda", zero=True)
    op = ConvTOp(torch.zeros(cin, cout, 2, 2, device="cuda"), torch.zeros(cout, device="cuda"))
    wl = torch.zeros(2, 2, cin, cout, device="cuda")
    geoms = [list(op._geom(x, out, ky, kx)) for ky in range(2) for kx in range(2)]

    def classes(gs, flags=0):
        g4 = host_i32([v for g in gs for v in g])
        call("mopa_conv2d_igemm_classes", x.p, ptr(wl), None, out.p, ctypes.addressof(g4), flags, stream())

    classes(geoms)
    empty = [list(g) for g in geoms]
    empty[3][15] = 0                                  # TH = 0: an empty class
    other = [list(g) for g in geoms]
    other[2][1] += 1                                  # IH: the classes do not share the input image
    for bad in (empty, other):
        with pytest.raises(RuntimeError):
            classes(bad)
    with pytest.raises(RuntimeError):
        classes(geoms, (1 + 1) << 8)                  # the 128 x 128 tile
    dw = torch.empty(cin, cout, 2, 2, device="cuda")
    small = new_img(B, 2 * H - 1, 2 * W, cout, "cuda", zero=True)    # an output gradient smaller than 2H x 2W
    for gi, ok in ((out, True), (small, False)):
        g = op._geom(x, gi, 0, 0)
        ws = workspace.get(query("mopa_convt_wgrad_workspace_bytes", ctypes.addressof(g)), dw.device)
        args = (x.p, gi.p, ptr(dw), ctypes.addressof(g), 0, ptr(ws), ws.numel(), stream())
        if ok:
            call("mopa_convt_bwd_weight", *args)
            with pytest.raises(RuntimeError):         # workspace too small
                call("mopa_convt_bwd_weight", *args[:6], 256, stream())
        else:
            with pytest.raises(RuntimeError):
                call("mopa_convt_bwd_weight", *args)
    torch.cuda.synchronize()


def _network_run(monkeypatch, on, state):
    from mopa_amd import dense2d
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d
    from mopa_amd.optim import FlatAdam
    monkeypatch.setattr(dense2d, "CONV_CLASSES", on)
    monkeypatch.setattr(dense2d, "GRAPH_2D", False)
    monkeypatch.setattr(dense2d, "NATIVE_2D", True)
    rng = np.random.Generator(np.random.PCG64(23))
    H, W, n = 64, 96, 150
    batch = {"img": torch.from_numpy(rng.random((2, 3, H, W), dtype=np.float32)),
             "img_indices": [np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1).astype(np.int64) for _ in range(2)],
             "bn_groups": 2}
    m = build_model_2d(default_cfg())[0]
    m.load_state_dict(state)
    m = m.cuda().train()
    calls = _logged(monkeypatch, dense2d)
    for k in dense2d.GRAPH_STATS:
        dense2d.GRAPH_STATS[k] = 0
    opt = FlatAdam(m.parameters(), lr=1e-3)   # (attached gradient buffers: a backward pass without them is not replayed; no step is taken)
    for _ in range(3):                         # eager, recorded, replayed: the last pass's results
        opt.zero_grad()
        o = m(batch)
        g = torch.Generator(device="cuda").manual_seed(1)
        sum((o[k] * torch.randn(o[k].shape, device="cuda", generator=g)).sum() for k in ("seg_logit", "seg_logit2")).backward()
    torch.cuda.synchronize()
    return ({k: o[k].detach().clone() for k in ("seg_logit", "seg_logit2")},
            {n_: p.grad.clone() for n_, p in m.named_parameters() if p.grad is not None}, list(calls), dict(dense2d.GRAPH_STATS))


def test_network_with_and_without_the_one_launch_classes(monkeypatch):
    """Two fresh Net2DSeg models from one state_dict, 2 images of 64 x 96 with 300 points, bn_groups = 2, forward and backward three
    times (walked, recorded, replayed): outputs and every gradient bit for bit, and the command list with the new entry points replays."""
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d
    torch.manual_seed(9)
    state = {k: v.clone() for k, v in build_model_2d(default_cfg())[0].state_dict().items()}
    oa, ga, ca, _ = _network_run(monkeypatch, False, state)
    ob, gb, cb, st = _network_run(monkeypatch, True, state)
    assert "mopa_conv2d_igemm_classes" not in ca and "mopa_convt_bwd_weight" not in ca
    assert cb.count("mopa_conv2d_igemm_classes") > 0 and cb.count("mopa_convt_bwd_weight") > 0
    assert st["recorded"] > 0 and st["forward_replays"] > 0 and st["backward_replays"] > 0, st
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    assert set(ga) == set(gb) and len(ga) > 0
    for n in ga:
        assert torch.equal(ga[n], gb[n]), (n, float((ga[n] - gb[n]).abs().max()))
    assert all(float(gb[n].abs().max()) > 0 for n in gb if "dec_t_conv" in n and n.endswith("weight"))
