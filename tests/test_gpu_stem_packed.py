"""The stem over its 147 real taps instead of 7 x 32 padded slots: the forward from an image strip (mopa_stem_fwd) against the implicit
GEMM it replaces, and the strip weight gradient's packed row tiles (mopa_stem_bwd_weight2 / mopa_stem_bwd_weight_bn2 with the
parameter layout) against the first form -- bit for bit, at grids small enough to hit every edge.

Shapes are OUTPUT grids B x Hp x Wp; the image tensor is B x (Hp + 6) x (Wp + 8) x 4 as mopa_img_to_nhwc4 leaves it: channel 3 zero,
a zero frame of 3 pixels left and above, 5 right, 3 below.

What is NOT asserted: that the padding positions (kw = 7, c = 3) of the [7][2][16][64] result are zero.  They are sums over real
pixels in the first form (pixel 7 of a tap is the image pixel right of the window), tests/test_gpu_stem_bwd.py holds that layout to
the first form's bits at every position, and so does this file; the packed tiles therefore serve the parameter layout only, where
the reduction drops those rows.  The zeros the packed kernel writes are checked where they are: in the slabs."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("MOPA_CONV2D_MFMA", "1") == "0",
                                 reason="the stem's MFMA kernels are switched off (MOPA_CONV2D_MFMA=0)")]

# B, Hp, Wp, G: the smallest grid; one forward chunk per row (two 32-pixel tiles, the second short), shorter than the weight
# gradient's 64-pixel chunk; chunks of 64 + 16; 64 + 64 + 16 (forward: 128 + 16) and three BatchNorm groups; weight-gradient blocks
# that end in mid-row (forward: 128 + 80)
SHAPES = [(1, 16, 16, 1), (2, 32, 48, 2), (2, 16, 80, 2), (3, 16, 144, 3), (1, 48, 208, 1)]
SLAB = 224 * 64   # floats of one weight-gradient slab [7][2][16][64]


def _geom(B, Hp, Wp, ld_out):
    from mopa_amd.dense2d import _geom as geom
    return geom(B=B, IH=Hp + 6, IW=Wp + 8, OHl=Hp, OWl=Wp, OHa=Hp, OWa=Wp, IDX=4, TH=7, TW=2, KWF=2, Cin=16, Cout=64, ld_in=4,
                ld_out=ld_out)


def _image(rng, B, Hp, Wp):
    """(img (B, 3, Hp, Wp) on the host, its NHWC4 frame on the device)."""
    from mopa_amd._lib import call, ptr, stream
    img = torch.from_numpy(rng.standard_normal((B, 3, Hp, Wp)).astype(np.float32))
    x4 = torch.full((B, Hp + 6, Wp + 8, 4), float("nan"), device="cuda")
    call("mopa_img_to_nhwc4", ptr(img.cuda()), B, Hp, Wp, Hp, Wp, ptr(x4), stream())
    return img, x4


def _weight(rng):
    """(w (64, 3, 7, 7) on the host, its [7][2][16][64] form on the device)."""
    from mopa_amd._lib import call, ptr, stream
    w = torch.from_numpy((rng.standard_normal((64, 3, 7, 7)) * 0.05).astype(np.float32))
    w1 = torch.full((7, 2, 16, 64), float("nan"), device="cuda")
    call("mopa_conv2d_stem_relayout", ptr(w.cuda()), ptr(w1), 64, 0, 0, stream())
    return w, w1


def _rand(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()


# ---------------------------------------------------------------------------------------------------------------- forward
# (the listed grids and one of 1,035 chunks: two per block, blocks that cross rows and images)
@pytest.mark.parametrize("B,Hp,Wp", [s[:3] for s in SHAPES] + [(3, 115, 272)])
@pytest.mark.parametrize("ld_out", [64, 128])
def test_forward_has_the_bits_of_the_implicit_gemm(B, Hp, Wp, ld_out):
    from mopa_amd._lib import call, ptr, stream
    rng = np.random.Generator(np.random.PCG64(2800 + Wp + ld_out))
    _, x4 = _image(rng, B, Hp, Wp)
    _, w1 = _weight(rng)
    geom = _geom(B, Hp, Wp, ld_out)
    old = torch.full((B * Hp * Wp, ld_out), -7.0, device="cuda")
    new = old.clone()
    call("mopa_conv2d_igemm", ptr(x4), ptr(w1), None, ptr(old), ctypes.addressof(geom), 0, stream())
    call("mopa_stem_fwd", ptr(x4), ptr(w1), ptr(new), ctypes.addressof(geom), stream())
    assert torch.equal(old.view(torch.int32), new.view(torch.int32)), float((old - new).abs().max())
    assert float(new[:, :64].abs().max()) > 0 and bool((new[:, 64:] == -7.0).all())   # (the right half of a join buffer stays)


@pytest.mark.parametrize("B,Hp,Wp", [s[:3] for s in SHAPES])
def test_forward_vs_fp64_conv(B, Hp, Wp):
    """Against float64 F.conv2d (7x7, padding 3) under the bound of the stem's kernel test in tests/test_gpu_2d.py
    (test_stem_dgrad_image_kernel_vs_torch: rtol 1e-4, atol 1e-4 of the largest value)."""
    from mopa_amd._lib import call, ptr, stream
    rng = np.random.Generator(np.random.PCG64(2900 + Wp))
    img, x4 = _image(rng, B, Hp, Wp)
    w, w1 = _weight(rng)
    geom = _geom(B, Hp, Wp, 64)
    out = torch.full((B * Hp * Wp, 64), float("nan"), device="cuda")
    call("mopa_stem_fwd", ptr(x4), ptr(w1), ptr(out), ctypes.addressof(geom), stream())
    ref = F.conv2d(img.double(), w.double(), None, 1, 3).permute(0, 2, 3, 1).reshape(B * Hp * Wp, 64).numpy()
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(ref).max())))


def test_forward_refuses_what_is_not_the_dense_stem():
    from mopa_amd._lib import call, ptr, stream
    from mopa_amd.dense2d import _geom as geom
    rng = np.random.Generator(np.random.PCG64(2950))
    _, x4 = _image(rng, 2, 16, 16)
    _, w1 = _weight(rng)
    out = torch.empty(2 * 16 * 16, 64, device="cuda")
    strided = geom(B=2, IH=22, IW=24, OHl=8, OWl=8, OHa=8, OWa=8, IS=2, IDX=4, TH=7, TW=2, KWF=2, Cin=16, Cout=64, ld_in=4, ld_out=64)
    narrow = _geom(2, 16, 16, 60)
    for g in (strided, narrow):
        with pytest.raises(RuntimeError):
            call("mopa_stem_fwd", ptr(x4), ptr(w1), ptr(out), ctypes.addressof(g), stream())
    with pytest.raises(RuntimeError):   # a weight that is not 16-byte aligned
        call("mopa_stem_fwd", ptr(x4), ptr(w1) + 4, ptr(out), ctypes.addressof(_geom(2, 16, 16, 64)), stream())


# ---------------------------------------------------------------------------------------------------------------- weight gradient
def _ws(geom):
    from mopa_amd._lib import query, workspace
    nbytes = query("mopa_conv2d_wgrad_workspace_bytes", ctypes.addressof(geom))
    return workspace.get(nbytes, torch.device("cuda", torch.cuda.current_device())), nbytes


def _bn_inputs(rng, rows, G):
    stats = torch.empty(G, 4, 64, device="cuda")
    stats[:, 0] = _rand(rng, G, 64)                      # scale (either sign)
    stats[:, 1] = _rand(rng, G, 64) * 0.5                # shift
    stats[:, 2] = _rand(rng, G, 64) * 0.3                # mean
    stats[:, 3] = _rand(rng, G, 64).abs() + 0.5          # 1 / std
    return stats, _rand(rng, G, 2, 64) * 0.1, _rand(rng, rows, 64)


def _padding_rows():
    """Mask (224,) of a slab's rows that carry no tap: channel 3 of every pixel and pixel 7 of every filter row."""
    r = np.arange(224) % 32
    return torch.from_numpy((r % 4 == 3) | (r // 4 == 7))


def _check_slabs(ws, nbytes):
    """After a parameter-layout call the workspace holds the packed kernel's slabs: their padding rows are zeros, a real row is not."""
    ns = nbytes // (SLAB * 4)
    slabs = ws[:ns * SLAB * 4].view(torch.float32).view(ns, 224, 64).cpu()
    pad = _padding_rows()
    assert int(pad.sum()) == 224 - 147
    assert bool((slabs[:, pad] == 0).all())
    assert bool((slabs[:, ~pad] != 0).any(dim=2).all())
    return ns


@pytest.mark.parametrize("B,Hp,Wp,G", SHAPES)
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_weight_gradient_has_the_bits_of_the_first_form(B, Hp, Wp, G, flags):
    """mopa_stem_bwd_weight2 == mopa_conv2d_bwd_weight (+ mopa_conv2d_stem_relayout for the parameter layout), fresh and accumulating."""
    from mopa_amd._lib import call, ptr, stream
    rng = np.random.Generator(np.random.PCG64(3000 + Wp + flags))
    _, x4 = _image(rng, B, Hp, Wp)
    dy = _rand(rng, B * Hp * Wp, 128)
    geom = _geom(B, Hp, Wp, 128)
    ws, nbytes = _ws(geom)
    acc, param = flags & 1, flags >> 1
    base = _rand(rng, 64, 3, 7, 7) if param else _rand(rng, 7, 2, 16, 64)
    old, new = base.clone(), base.clone()
    if param:
        dwl = torch.empty(7, 2, 16, 64, device="cuda")
        call("mopa_conv2d_bwd_weight", ptr(x4), ptr(dy), ptr(dwl), ctypes.addressof(geom), 0, ptr(ws), nbytes, stream())
        call("mopa_conv2d_stem_relayout", ptr(dwl), ptr(old), 64, 1, acc, stream())
    else:
        call("mopa_conv2d_bwd_weight", ptr(x4), ptr(dy), ptr(old), ctypes.addressof(geom), acc, ptr(ws), nbytes, stream())
    ws.fill_(255)   # (NaN bit patterns: what the slabs hold afterwards was written by this call)
    call("mopa_stem_bwd_weight2", ptr(x4), ptr(dy), ptr(new), ctypes.addressof(geom), flags, ptr(ws), nbytes, stream())
    assert torch.equal(old, new), float((old - new).abs().max())
    assert not torch.equal(new, base)
    if param:
        ns = _check_slabs(ws, nbytes)
        if (B, Hp, Wp) == (1, 48, 208):   # wgrad_split: ceil(M / 1152) slabs of ceil(M / ns) pixels rounded up to 16
            mps = -(-(-(B * Hp * Wp // -ns)) // 16) * 16
            assert ns == 9 and mps == 1120 and mps % Wp != 0   # blocks end in mid-row


@pytest.mark.parametrize("B,Hp,Wp,G", SHAPES)
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_weight_gradient_with_the_batchnorm_backward_has_the_bits_of_the_first_form(B, Hp, Wp, G, training, flags):
    """mopa_stem_bwd_weight_bn2 == mopa_stem_bwd_weight_bn (+ relayout), G groups, dy in the left half of a 128-wide buffer."""
    from mopa_amd._lib import call, ptr, stream
    rng = np.random.Generator(np.random.PCG64(3100 + Wp + flags + 4 * training))
    _, x4 = _image(rng, B, Hp, Wp)
    dy = _rand(rng, B * Hp * Wp, 128)
    stats, coef, xbn = _bn_inputs(rng, B * Hp * Wp, G)
    geom = _geom(B, Hp, Wp, 128)
    ws, nbytes = _ws(geom)
    acc, param = flags & 1, flags >> 1
    base = _rand(rng, 64, 3, 7, 7) if param else _rand(rng, 7, 2, 16, 64)
    old, new = base.clone(), base.clone()
    dwl = torch.empty(7, 2, 16, 64, device="cuda") if param else old
    call("mopa_stem_bwd_weight_bn", ptr(x4), ptr(dy), 128, ptr(xbn), 64, ptr(stats), ptr(coef), G, training, ptr(dwl),
         ctypes.addressof(geom), 0 if param else acc, ptr(ws), nbytes, stream())
    if param:
        call("mopa_conv2d_stem_relayout", ptr(dwl), ptr(old), 64, 1, acc, stream())
    ws.fill_(255)   # (NaN bit patterns: what the slabs hold afterwards was written by this call)
    call("mopa_stem_bwd_weight_bn2", ptr(x4), ptr(dy), 128, ptr(xbn), 64, ptr(stats), ptr(coef), G, training, ptr(new),
         ctypes.addressof(geom), flags, ptr(ws), nbytes, stream())
    assert torch.equal(old, new), float((old - new).abs().max())
    assert not torch.equal(new, base)
    if param:
        _check_slabs(ws, nbytes)


# ---------------------------------------------------------------------------------------------------------------- network
def _network_run(monkeypatch, packed, state, replay):
    from mopa_amd import dense2d
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d
    from mopa_amd.optim import FlatAdam
    monkeypatch.setattr(dense2d, "STEM_PACKED", packed)
    monkeypatch.setattr(dense2d, "STEM_BWD2_MIN_PIXELS", 0)
    monkeypatch.setattr(dense2d, "GRAPH_2D", False)
    monkeypatch.setattr(dense2d, "NATIVE_2D", replay)
    rng = np.random.Generator(np.random.PCG64(3200))
    H, W, n = 64, 96, 150
    batch = {"img": torch.from_numpy(rng.random((2, 3, H, W), dtype=np.float32)), "bn_groups": 2,
             "img_indices": [np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1).astype(np.int64) for _ in range(2)]}
    torch.manual_seed(9)
    m = build_model_2d(default_cfg())[0]
    m.load_state_dict(state)
    m = m.cuda().train()
    calls = []
    inner = dense2d.call
    monkeypatch.setattr(dense2d, "call", lambda name, *a: (calls.append(name), inner(name, *a))[1])
    for k in dense2d.GRAPH_STATS:
        dense2d.GRAPH_STATS[k] = 0
    opt = FlatAdam(m.parameters(), lr=1e-3)   # (attached gradient buffers: a backward pass without them is not replayed; no step is taken)
    for _ in range(3 if replay else 1):       # eager, recorded, replayed: the last pass's results
        opt.zero_grad()
        o = m(batch)
        g = torch.Generator(device="cuda").manual_seed(1)
        sum((o[k] * torch.randn(o[k].shape, device="cuda", generator=g)).sum() for k in ("seg_logit", "seg_logit2")).backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(dense2d, "call", inner)
    return (o["seg_logit"].detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, calls,
            dict(dense2d.GRAPH_STATS))


@pytest.mark.parametrize("replay", [False, True])
def test_network_with_and_without_the_packed_stem(replay, monkeypatch):
    """Two Net2DSeg from one state_dict on 2 images of 64 x 96 with 300 points, two BatchNorm groups, the strip weight gradient at
    every size: switch on against off, logits and every parameter gradient bit for bit, walked from Python and through the native
    command list (recorded in the second pass, replayed in the third)."""
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d
    torch.manual_seed(28)
    state = {k: v.clone() for k, v in build_model_2d(default_cfg())[0].state_dict().items()}
    la, ga, ca, _ = _network_run(monkeypatch, False, state, replay)
    lb, gb, cb, st = _network_run(monkeypatch, True, state, replay)
    assert "mopa_stem_fwd" not in ca and ca.count("mopa_stem_bwd_weight_bn2") == cb.count("mopa_stem_bwd_weight_bn2") >= 1
    # every forward pass walked from Python (a replayed one makes no call) sends the stem through the new entry point, nothing else moves
    assert cb.count("mopa_stem_fwd") == ca.count("mopa_conv2d_igemm") - cb.count("mopa_conv2d_igemm") == (2 if replay else 1)
    if replay:
        assert st["forward_replays"] >= 1 and st["backward_replays"] >= 1, st
    assert torch.equal(la, lb)
    assert set(ga) == set(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), (k, float((ga[k] - gb[k]).abs().max()))
    assert float(gb["net_2d.conv1.weight"].abs().max()) > 0
