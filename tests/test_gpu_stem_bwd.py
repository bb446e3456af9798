"""The second form of the image branch's backward tail (dense2d.STEM_BWD2): the stem's weight gradient from an image strip
(mopa_stem_bwd_weight2 / mopa_stem_bwd_weight_bn2), the max-pool's backward inside the stem BatchNorm's sums pass
(mopa_bn_bwd_sums_groups_pool) and the slab reduction that writes the parameter gradient's layout -- every one of them against the
calls it replaces, bit for bit.

The stem is 7x7 / stride 1 / padding 3 on the zero-padded NHWC4 image (mopa_img_to_nhwc4), so its output grid is the padded image's:
the shapes below are OUTPUT grids (B x OH x OW, M = B * OH * OW pixels), the image tensor is B x (OH + 6) x (OW + 8) x 4."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("MOPA_CONV2D_MFMA", "1") == "0",
                                 reason="the stem's MFMA weight gradients are switched off (MOPA_CONV2D_MFMA=0)")]

# B, OH, OW: less than one chunk; one slab, odd width, ragged end; 4 slabs of 912 with the last short, rows and images change inside
# chunks; the network test's pooled and full grids (16 slabs of 1120: slab borders inside rows)
STEM_SHAPES = [(1, 3, 5), (2, 19, 23), (3, 27, 45), (2, 40, 56), (2, 80, 112)]


def _rand(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()


def _stem_problem(B, OH, OW, ld_dy, seed):
    from mopa_amd.dense2d import _geom
    rng = np.random.Generator(np.random.PCG64(seed))
    x4 = _rand(rng, B, OH + 6, OW + 8, 4)
    dy = _rand(rng, B * OH * OW, ld_dy)
    geom = _geom(B=B, IH=OH + 6, IW=OW + 8, OHl=OH, OWl=OW, OHa=OH, OWa=OW, IDX=4, TH=7, TW=2, KWF=2, Cin=16, Cout=64, ld_in=4,
                 ld_out=ld_dy)
    return rng, x4, dy, geom


def _ws(geom):
    from mopa_amd._lib import query, workspace
    nbytes = query("mopa_conv2d_wgrad_workspace_bytes", ctypes.addressof(geom))
    return workspace.get(nbytes, torch.device("cuda", torch.cuda.current_device())), nbytes


@pytest.mark.parametrize("B,OH,OW", STEM_SHAPES)
@pytest.mark.parametrize("ld_dy", [64, 128])
def test_strip_weight_gradient_has_the_bits_of_the_im2col_kernel(B, OH, OW, ld_dy):
    """mopa_stem_bwd_weight2 == mopa_conv2d_bwd_weight on the stem geometry (fresh and accumulating), same workspace."""
    from mopa_amd._lib import call, ptr, stream
    rng, x4, dy, geom = _stem_problem(B, OH, OW, ld_dy, 100 + OW)
    ws, nbytes = _ws(geom)
    base = _rand(rng, 7, 2, 16, 64)
    for acc in (0, 1):
        old, new = base.clone(), base.clone()
        call("mopa_conv2d_bwd_weight", ptr(x4), ptr(dy), ptr(old), ctypes.addressof(geom), acc, ptr(ws), nbytes, stream())
        call("mopa_stem_bwd_weight2", ptr(x4), ptr(dy), ptr(new), ctypes.addressof(geom), acc, ptr(ws), nbytes, stream())
        assert torch.equal(old, new), (acc, float((old - new).abs().max()))
    assert float(new.abs().max()) > 0
    # the same workspace query serves both: its size is accepted, one byte less is MOPA_ERR_WORKSPACE for both
    for name in ("mopa_conv2d_bwd_weight", "mopa_stem_bwd_weight2"):
        with pytest.raises(RuntimeError):
            call(name, ptr(x4), ptr(dy), ptr(new), ctypes.addressof(geom), 0, ptr(ws), nbytes - 1, stream())


def _bn_inputs(rng, rows, G):
    stats = torch.empty(G, 4, 64, device="cuda")
    stats[:, 0] = _rand(rng, G, 64)                      # scale (either sign)
    stats[:, 1] = _rand(rng, G, 64) * 0.5                # shift
    stats[:, 2] = _rand(rng, G, 64) * 0.3                # mean
    stats[:, 3] = _rand(rng, G, 64).abs() + 0.5          # 1 / std
    coef = _rand(rng, G, 2, 64) * 0.1
    xbn = _rand(rng, rows, 64)
    return stats, coef, xbn


@pytest.mark.parametrize("B,OH,OW", STEM_SHAPES)
@pytest.mark.parametrize("training", [1, 0])
def test_strip_weight_gradient_with_the_batchnorm_backward_in_its_loader(B, OH, OW, training):
    """mopa_stem_bwd_weight_bn2 == mopa_stem_bwd_weight_bn: dy in the left half of a 128-wide buffer, x with rows of 64, every group
    count the batch allows, training and eval."""
    from mopa_amd._lib import call, ptr, stream
    rng, x4, dy, geom = _stem_problem(B, OH, OW, 128, 200 + OW)
    ws, nbytes = _ws(geom)
    for G in (g for g in (1, 2, 3) if B % g == 0):
        stats, coef, xbn = _bn_inputs(rng, B * OH * OW, G)
        old, new = torch.empty(7, 2, 16, 64, device="cuda"), torch.empty(7, 2, 16, 64, device="cuda")
        call("mopa_stem_bwd_weight_bn", ptr(x4), ptr(dy), 128, ptr(xbn), 64, ptr(stats), ptr(coef), G, training, ptr(old),
             ctypes.addressof(geom), 0, ptr(ws), nbytes, stream())
        call("mopa_stem_bwd_weight_bn2", ptr(x4), ptr(dy), 128, ptr(xbn), 64, ptr(stats), ptr(coef), G, training, ptr(new),
             ctypes.addressof(geom), 0, ptr(ws), nbytes, stream())
        assert torch.equal(old, new), (G, float((old - new).abs().max()))
        assert float(new.abs().max()) > 0


def test_strip_weight_gradient_vs_fp64_autograd():
    """The parameter-layout gradient (flags bit 1) against float64 autograd of F.conv2d on the padded image; the bound of the stem's
    data-gradient test (tests/test_gpu_2d.py::test_stem_dgrad_image_kernel_vs_torch: rtol 1e-4, atol 1e-4 of the largest value)."""
    from mopa_amd._lib import call, ptr, stream
    B, OH, OW = 2, 19, 23
    rng, x4, dy, geom = _stem_problem(B, OH, OW, 64, 300)
    ws, nbytes = _ws(geom)
    dw = torch.empty(64, 3, 7, 7, device="cuda")
    call("mopa_stem_bwd_weight2", ptr(x4), ptr(dy), ptr(dw), ctypes.addressof(geom), 2, ptr(ws), nbytes, stream())
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    img = x4.cpu().double()[..., :3].permute(0, 3, 1, 2)              # (B, 3, OH + 6, OW + 8): the padding is part of the tensor
    y = F.conv2d(img, w)[..., :OW]                                    # (B, 64, OH, OW)
    (y * dy.cpu().double().reshape(B, OH, OW, 64).permute(0, 3, 1, 2)).sum().backward()
    ref = w.grad.numpy()
    np.testing.assert_allclose(dw.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("acc", [0, 1])
def test_slab_reduction_into_the_parameter_layout(acc):
    """flags bit 1 of the new entry points == ordered reduction into [7][2][16][64] + mopa_conv2d_stem_relayout(inverse), with and
    without accumulation into the parameter gradient (3 x 27 x 45: four slabs)."""
    from mopa_amd._lib import call, ptr, stream
    B, OH, OW = 3, 27, 45
    rng, x4, dy, geom = _stem_problem(B, OH, OW, 128, 400)
    ws, nbytes = _ws(geom)
    stats, coef, xbn = _bn_inputs(rng, B * OH * OW, 3)
    base = _rand(rng, 64, 3, 7, 7)
    for bn in (False, True):
        ref, got, dwl = base.clone(), base.clone(), torch.empty(7, 2, 16, 64, device="cuda")
        if bn:
            call("mopa_stem_bwd_weight_bn", ptr(x4), ptr(dy), 128, ptr(xbn), 64, ptr(stats), ptr(coef), 3, 1, ptr(dwl),
                 ctypes.addressof(geom), 0, ptr(ws), nbytes, stream())
        else:
            call("mopa_conv2d_bwd_weight", ptr(x4), ptr(dy), ptr(dwl), ctypes.addressof(geom), 0, ptr(ws), nbytes, stream())
        call("mopa_conv2d_stem_relayout", ptr(dwl), ptr(ref), 64, 1, acc, stream())
        if bn:
            call("mopa_stem_bwd_weight_bn2", ptr(x4), ptr(dy), 128, ptr(xbn), 64, ptr(stats), ptr(coef), 3, 1, ptr(got),
                 ctypes.addressof(geom), acc | 2, ptr(ws), nbytes, stream())
        else:
            call("mopa_stem_bwd_weight2", ptr(x4), ptr(dy), ptr(got), ctypes.addressof(geom), acc | 2, ptr(ws), nbytes, stream())
        assert torch.equal(ref, got), (bn, float((ref - got).abs().max()))
        assert not torch.equal(got, base)


# pre-pool maps B x H x W and group counts: odd in both directions with every border; the network test's; three groups
POOL_SHAPES = [(1, 5, 7, 1), (2, 40, 56, 2), (3, 27, 45, 3)]


@pytest.mark.parametrize("B,H,W,G", POOL_SHAPES)
@pytest.mark.parametrize("acc_dy", [1, 0])
@pytest.mark.parametrize("acc_params", [0, 1])
@pytest.mark.parametrize("peaks", [False, True])
def test_maxpool_backward_inside_the_batchnorm_sums_pass(B, H, W, G, acc_dy, acc_params, peaks):
    """mopa_bn_bwd_sums_groups_pool == mopa_maxpool3x3s2_bwd then mopa_bn_bwd_sums_groups: the written tensor (left half of a 128-wide
    buffer, pre-filled or fresh; its right half untouched), dgamma, dbeta and coef.  peaks: pixels (1, 1) mod 4 carry the maximum of
    all four windows over them, so their sum has four terms."""
    from mopa_amd._lib import call, ptr, query, stream, workspace
    rng = np.random.Generator(np.random.PCG64(500 + W + 2 * acc_dy + acc_params))
    rows, OH, OW = B * H * W, (H + 1) // 2, (W + 1) // 2
    stats, _, x = _bn_inputs(rng, rows, G)
    if peaks:
        stats[:, 0] = stats[:, 0].abs() + 0.5
        xv = x.view(B, H, W, 64)
        xv[:, 1::4, 1::4] = 50.0 + _rand(rng, *xv[:, 1::4, 1::4].shape).abs()
    pooled, amax = torch.empty(B * OH * OW, 64, device="cuda"), torch.empty(B * OH * OW * 64, dtype=torch.uint8, device="cuda")
    call("mopa_maxpool3x3s2_fwd_bn", ptr(x), 64, B, H, W, 64, ptr(stats), G, ptr(pooled), 64, ptr(amax), stream())
    if peaks:   # pixel (1, 1) is tap (2, 2) of window (0, 0), (2, 0) of (0, 1), (0, 2) of (1, 0) and (0, 0) of (1, 1)
        a = amax.view(B, OH, OW, 64)
        assert all(bool((a[:, oy, ox] == tap).all()) for oy, ox, tap in ((0, 0, 8), (0, 1, 6), (1, 0, 2), (1, 1, 0)))
    dpool = _rand(rng, B * OH * OW, 64)
    base = _rand(rng, rows, 128)
    if not acc_dy:
        base[:, :64] = float("nan")   # a fresh destination is written, never read
    pg = _rand(rng, 2, 64)
    nbytes = query("mopa_bnrelu_rows_workspace_bytes", rows, 64)
    ws = workspace.get(nbytes, x.device)
    n = rows // G
    old, new = base.clone(), base.clone()
    og, ng, oc, nc = pg.clone(), pg.clone(), torch.empty(G, 2, 64, device="cuda"), torch.empty(G, 2, 64, device="cuda")
    call("mopa_maxpool3x3s2_bwd", ptr(dpool), 64, ptr(amax), B, H, W, 64, ptr(old), 128, acc_dy, stream())
    call("mopa_bn_bwd_sums_groups", ptr(old), 128, ptr(x), 64, rows, 64, G, n, 2 * n, ptr(stats), 0.0, 1, None, 0, ptr(og), ptr(og, 64),
         acc_params, ptr(oc), ptr(ws), nbytes, stream())
    call("mopa_bn_bwd_sums_groups_pool", ptr(dpool), 64, ptr(amax), B, H, W, ptr(new), 128, acc_dy, ptr(x), 64, 64, G, ptr(stats), 0.0, 1,
         ptr(ng), ptr(ng, 64), acc_params, ptr(nc), ptr(ws), nbytes, stream())
    assert not bool(torch.isnan(new[:, :64]).any())
    assert torch.equal(old.view(torch.int32), new.view(torch.int32))
    assert torch.equal(og, ng) and torch.equal(oc, nc)
    assert float(ng.abs().max()) > 0


def test_the_new_entry_points_refuse_what_the_old_ones_refuse():
    from mopa_amd._lib import call, ptr, query, stream, workspace
    from mopa_amd.dense2d import _geom
    rng, x4, dy, geom = _stem_problem(2, 8, 12, 64, 600)
    ws, nbytes = _ws(geom)
    dw = torch.empty(7, 2, 16, 64, device="cuda")
    strided = _geom(B=2, IH=14, IW=20, OHl=4, OWl=6, OHa=4, OWa=6, IS=2, IDX=4, TH=7, TW=2, KWF=2, Cin=16, Cout=64, ld_in=4, ld_out=64)
    with pytest.raises(RuntimeError):   # not the dense stride-1 stem: mopa_conv2d_bwd_weight's business
        call("mopa_stem_bwd_weight2", ptr(x4), ptr(dy), ptr(dw), ctypes.addressof(strided), 0, ptr(ws), nbytes, stream())
    stats, coef, xbn = _bn_inputs(rng, 2 * 8 * 12, 1)
    for G, ld in ((3, 64), (1, 60)):    # groups that do not divide the batch; a row stride below the channel count
        with pytest.raises(RuntimeError):
            call("mopa_stem_bwd_weight_bn2", ptr(x4), ptr(dy), ld, ptr(xbn), 64, ptr(stats), ptr(coef), G, 1, ptr(dw),
                 ctypes.addressof(geom), 0, ptr(ws), nbytes, stream())
    rows = 2 * 8 * 12
    pb = query("mopa_bnrelu_rows_workspace_bytes", rows, 64)
    pws = workspace.get(pb, x4.device)
    amax = torch.zeros(2 * 4 * 6 * 64, dtype=torch.uint8, device="cuda")
    dpool, dest, pg, co = _rand(rng, 2 * 4 * 6, 64), _rand(rng, rows, 64), _rand(rng, 2, 64), torch.empty(1, 2, 64, device="cuda")
    for C, G, ld in ((62, 1, 64), (64, 3, 64), (64, 1, 60)):
        with pytest.raises(RuntimeError):
            call("mopa_bn_bwd_sums_groups_pool", ptr(dpool), 64, ptr(amax), 2, 8, 12, ptr(dest), ld, 0, ptr(xbn), 64, C, G, ptr(stats), 0.0, 1,
                 ptr(pg), ptr(pg, 64), 0, ptr(co), ptr(pws), pb, stream())


def _network_run(monkeypatch, parts, groups, training, replay, want_dimg=False, min_pixels=0):
    from mopa_amd import dense2d, synth
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d
    monkeypatch.setattr(dense2d, "STEM_BWD2", frozenset(parts))
    if min_pixels is not None:
        monkeypatch.setattr(dense2d, "STEM_BWD2_MIN_PIXELS", min_pixels)
    monkeypatch.setattr(dense2d, "GRAPH_2D", False)
    monkeypatch.setattr(dense2d, "NATIVE_2D", replay)
    batch = synth.make_batch(2 * groups, H=80, W=112)
    if groups > 1:
        batch["bn_groups"] = groups
    if want_dimg:
        batch["img"] = batch["img"].cuda().requires_grad_(True)
    torch.manual_seed(9)
    m = build_model_2d(default_cfg())[0].cuda()
    m = m.train() if training else m.eval()
    calls = []
    inner = dense2d.call
    monkeypatch.setattr(dense2d, "call", lambda name, *a: (calls.append(name), inner(name, *a))[1])
    for k in dense2d.GRAPH_STATS:
        dense2d.GRAPH_STATS[k] = 0
    from mopa_amd.optim import FlatAdam
    opt = FlatAdam(m.parameters(), lr=1e-3)   # (attached gradient buffers: a backward pass without them is not replayed; no step is taken)
    for _ in range(3 if replay else 1):       # eager, recorded, replayed: the last pass's results
        opt.zero_grad()
        o = m(batch)
        g = torch.Generator(device="cuda").manual_seed(1)
        sum((o[k] * torch.randn(o[k].shape, device="cuda", generator=g)).sum() for k in ("seg_logit", "seg_logit2")).backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(dense2d, "call", inner)
    return (o["seg_logit"].detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, calls,
            dict(dense2d.GRAPH_STATS))


NEW_CALLS = ("mopa_bn_bwd_sums_groups_pool", "mopa_stem_bwd_weight_bn2")
OLD_CALLS = ("mopa_maxpool3x3s2_bwd", "mopa_stem_bwd_weight_bn", "mopa_conv2d_stem_relayout")


@pytest.mark.parametrize("groups,training", [(1, True), (2, True), (1, False), (2, False)])
@pytest.mark.parametrize("replay", [False, True])
def test_network_with_and_without_the_second_stem_backward(groups, training, replay, monkeypatch):
    """Net2DSeg on 2 G images of 80 x 112, switch on against off: logits and every parameter gradient bit for bit, walked from Python
    and through the native command list (recorded in the second pass, replayed in the third); the call log names the entry points."""
    la, ga, ca, _ = _network_run(monkeypatch, (), groups, training, replay)
    lb, gb, cb, st = _network_run(monkeypatch, ("wgrad", "pool"), groups, training, replay)
    passes = cb.count("mopa_stem_bwd_weight_bn2")   # backward passes walked from Python (a replayed one makes no call)
    assert passes == (1 if not replay else ca.count("mopa_stem_bwd_weight_bn"))
    if replay:   # the first pass is walked, the second is walked once more while it is recorded, then replayed; the third is a replay
        assert (st["backward_replays"], passes) == ((2, 2) if training else (0, 3)), (st, passes)   # (an eval-mode pass is never recorded)
    assert all(n not in ca for n in NEW_CALLS)
    assert all(cb.count(n) == passes for n in NEW_CALLS), {n: cb.count(n) for n in NEW_CALLS}
    assert "mopa_maxpool3x3s2_bwd" not in cb and "mopa_stem_bwd_weight_bn" not in cb
    # the forward pass still lays the stem's weights out (inverse = 0); the backward's relayout launch is gone
    assert cb.count("mopa_conv2d_stem_relayout") == ca.count("mopa_conv2d_stem_relayout") - ca.count("mopa_stem_bwd_weight_bn")
    assert torch.equal(la, lb)
    assert set(ga) == set(gb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), (n, float((ga[n] - gb[n]).abs().max()))
    assert float(gb["net_2d.conv1.weight"].abs().max()) > 0


@pytest.mark.parametrize("parts", [("wgrad",), ("pool",)])
def test_each_part_of_the_switch_alone(parts, monkeypatch):
    la, ga, _, _ = _network_run(monkeypatch, (), 2, True, False)
    lb, gb, cb, _ = _network_run(monkeypatch, parts, 2, True, False)
    assert (cb.count("mopa_stem_bwd_weight_bn2"), cb.count("mopa_bn_bwd_sums_groups_pool")) == (int("wgrad" in parts), int("pool" in parts))
    assert torch.equal(la, lb) and all(torch.equal(ga[n], gb[n]) for n in ga)


def test_gradient_wrt_the_image_keeps_the_first_form(monkeypatch):
    """want_dimg: the stem BatchNorm writes its input gradient (the image gradient reads it), so neither new entry point runs."""
    _, g, calls, _ = _network_run(monkeypatch, ("wgrad", "pool"), 1, True, False, want_dimg=True)
    assert all(n not in calls for n in NEW_CALLS)
    assert calls.count("mopa_maxpool3x3s2_bwd") == 1 and "mopa_stem_dgrad_image" in calls


def test_small_stem_grids_keep_the_first_form(monkeypatch):
    """Below dense2d.STEM_BWD2_MIN_PIXELS stem pixels (here 2 x 80 x 112 against the default 131,072) the tail keeps the first form."""
    from mopa_amd import dense2d
    assert 2 * 80 * 112 < dense2d.STEM_BWD2_MIN_PIXELS <= 304 * 480
    _, _, calls, _ = _network_run(monkeypatch, ("wgrad", "pool"), 1, True, False, min_pixels=None)
    assert all(n not in calls for n in NEW_CALLS)
    assert calls.count("mopa_stem_bwd_weight_bn") == 1 and calls.count("mopa_maxpool3x3s2_bwd") == 1
