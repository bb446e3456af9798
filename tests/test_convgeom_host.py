"""tests/_convgeom_reference.py on the CPU: the float64 restatement of conv2d.hip's index map must be torch's convolution on every
operator geometry of the case table, and every case must be able to show a one-defect kernel at ten times the GPU tolerance
(else its inputs are too degenerate to mean anything on the GPU).  No GPU, no HIP library."""
import pytest
import torch

import _convgeom_reference as cr

IGEMM_CASES = cr.igemm_cases()
WGRAD_CASES = cr.wgrad_cases()


def _igemm_all(P, defect=None, defect_class=-1):
    """Every class of the problem into one sentinel-filled output; defect: applied to one class only."""
    x, w = cr.flat(P.xw, P.xcol), P.w.double()
    bias = None if P.bias is None else P.bias.double()
    out = cr.flat(torch.full(P.out_shape, cr.OUT_SENTINEL), P.ocol)
    mask = torch.zeros(len(out), dtype=torch.bool)
    for i, g in enumerate(P.geoms):
        out = cr.igemm_ref(g, x, w, bias, out, False, defect if i == defect_class % len(P.geoms) else None)
        m = cr.touched(g, len(out))
        assert not bool((mask & m).any())   # classes never share an output element
        mask |= m
    return out, mask


def _expect_flat(P):
    """The torch result laid into the flat output (the dense columns of the wide buffer)."""
    wide = torch.full(P.out_shape, cr.OUT_SENTINEL, dtype=torch.float64)
    wide[:, P.ocol:P.ocol + P.expect.shape[1]] = P.expect
    return wide.reshape(-1)[P.ocol:]


@pytest.mark.parametrize("case", IGEMM_CASES, ids=cr.case_id)
def test_igemm_restatement_is_torch_and_sees_every_defect(case):
    P = cr.problem(*case)
    out, mask = _igemm_all(P)
    ref = _expect_flat(P)
    assert int(mask.sum()) > 0 and bool((out[~mask] == cr.OUT_SENTINEL).all())
    assert float((out[mask] - ref[mask]).abs().max()) <= 1e-12
    g0 = cr.fields(P.geoms[0])
    dense = torch.zeros(P.out_shape, dtype=torch.bool).reshape(-1)
    dense[P.ocol:] = mask
    dense = dense.reshape(P.out_shape)
    assert not bool(dense[:, :P.ocol].any()) and not bool(dense[:, P.ocol + g0.Cout:].any())
    if not P.name.startswith("dgrad1s2"):   # (the 1x1 stride-2 layer's backward-data has one class: odd pixels get nothing)
        assert bool(dense[:, P.ocol:P.ocol + g0.Cout].all())
    # the weight-gradient half on the same geometry: wgrad_ref is autograd's gradient of <operator(x, w), dy> in w (the operator
    # being torch's, as just shown), for every class and with dy in the output's own wide buffer
    x = cr.flat(P.xw, P.xcol)
    dy = torch.from_numpy(cr._rng(P.name + "dy").standard_normal(len(out)))
    for g in P.geoms:
        w = P.w.double().requires_grad_(True)
        (cr.igemm_ref(g, x, w, None, torch.zeros_like(out), False) * dy).sum().backward()
        assert float((cr.wgrad_ref(g, x, dy) - cr.tap_weights(cr.fields(g), w.grad)).abs().max()) <= 1e-12
    bound = cr.bound(ref[mask], P.role)
    for defect in cr.DEFECTS:
        if defect == "bias" and P.bias is None:
            continue
        for cls in range(len(P.geoms)):
            bad, _ = _igemm_all(P, defect, cls)
            # ("last_row" leaves the sentinel in place of a value)
            assert bool(((bad[mask] - ref[mask]).abs() > 10 * bound).any()), (defect, cls)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=cr.case_id)
def test_wgrad_restatement_is_autograd_and_sees_every_defect(case):
    P = cr.problem(*case)
    x, dy = cr.flat(P.xw, P.xcol), cr.flat(P.dyw, P.ocol)
    dw = cr.wgrad_ref(P.geoms[0], x, dy)
    real = getattr(P, "dw_real", torch.ones_like(dw, dtype=torch.bool))   # (the stem: the slots that are filter elements)
    assert float((dw - P.dw_expect)[real].abs().max()) <= 1e-12
    g = cr.fields(P.geoms[0])
    assert torch.equal(cr.oihw(dw), dw.permute(2, 1, 0)) and tuple(cr.oihw(dw).shape) == (g.Cout, g.Cin, g.TH * g.TW)
    if P.name.startswith("conv"):   # flags bit 1 is the parameter's own gradient tensor
        k = g.TH
        want = P.dw_expect.reshape(k, k, g.Cin, g.Cout).permute(3, 2, 0, 1)   # OIHW
        assert float((cr.oihw(dw).reshape(g.Cout, g.Cin, k, k) - want).abs().max()) <= 1e-12
    bound = cr.bound(dw, "wgrad")
    for defect in ("tap", "ix0", "last_row"):
        bad = cr.wgrad_ref(P.geoms[0], x, dy, defect)
        assert bool(((bad - dw).abs() > 10 * bound).any()), defect


def test_stem_restatement_of_the_layout_kernels():
    """img_to_nhwc4 / stem_relayout (the numpy forms of mopa_img_to_nhwc4 and mopa_conv2d_stem_relayout) carry the 7x7 convolution:
    already used by every stem case above; here the slots that are not filter elements are pinned down."""
    w = torch.arange(64 * 3 * 7 * 7, dtype=torch.float32).reshape(64, 3, 7, 7) + 1
    wl = cr.stem_relayout(w)
    assert tuple(wl.shape) == (7, 2, 16, 64)
    assert float(wl[2, 1, 4 * 1 + 2, 5]) == float(w[5, 2, 2, 5]) and float(wl[6, 0, 0, 63]) == float(w[63, 0, 6, 0])
    assert bool((wl[:, 1, 12:] == 0).all()) and bool((wl[:, :, 3::4] == 0).all())      # kw = 7 and the fourth channel
    x4 = cr.img_to_nhwc4(torch.ones(2, 3, 4, 5), 6, 8)
    assert tuple(x4.shape) == (2, 12, 16, 4) and float(x4.sum()) == 2 * 3 * 4 * 5
    assert bool((x4[:, 3:7, 3:8, :3] == 1).all())


def test_the_table_covers_what_it_promises():
    ms = sorted({g[0] * g[1] * g[2] for g in cr.GRIDS})
    assert ms == [1, 2, 63, 64, 65, 129, 255, 256, 257, 270] and (1, 1, 257) in cr.GRIDS
    assert any(g[0] == 3 for g in cr.GRIDS)
    assert {c[2] for c in IGEMM_CASES} == {16, 48, 64} and {c[3] for c in IGEMM_CASES} == {64, 128}
    assert sorted({g[0] * g[1] * g[2] for g in cr.WGRAD_GRIDS}) == [1, 15, 16, 17, 257, 513]
    assert sorted({c[1][0] * c[1][1] * c[1][2] for c in WGRAD_CASES if c[0] == "stem"}) == [1, 15, 16, 17, 257, 513, 1260, 2349]
    for kind in cr.KINDS:   # every operator meets a bias and a NULL where it takes one, and 128 output channels (the 128x128 tile)
        mine = [c for c in IGEMM_CASES if c[0] == kind]
        assert len(mine) == len(cr.GRIDS)
        if kind != "stem":
            assert {c[3] for c in mine} == {64, 128}
        if kind in cr.CONVS or kind == "convt":   # (a bias over two column tiles and in the 128-wide tile, and NULL there too)
            assert {(c[3], c[4]) for c in mine} == {(64, False), (64, True), (128, False), (128, True)}
        else:
            assert not any(c[4] for c in mine)
    # the stride-2 backward-data: four classes of four sizes at 7x9, fewer than four where the image has one row or column
    P = cr.problem("dgrad3s2", (2, 4, 5), 128, 64)
    assert [(cr.fields(g).OHl, cr.fields(g).OWl) for g in P.geoms] == [(4, 5), (4, 4), (3, 5), (3, 4)]
    assert len(cr.problem("dgrad3s2", (1, 1, 1), 64, 64).geoms) == 1 and len(cr.problem("dgrad1s2", (1, 8, 8), 64, 64).geoms) == 1
