"""The loss block of a merged pass (csrc/losses.hip: mopa_point_losses_seg_fwd / _bwd, mopa_amd/trainloss.py::point_losses_merged).

Every CE / KL scalar of every segment is compared BIT FOR BIT with mopa_point_losses_fwd on the segment's row slice, every gradient
row with mopa_point_losses_bwd on the slice (zeros where the segment has no term for a head); through the Python API with the sliced
``point_losses`` recipe under ``torch.equal``.  The entropy term is compared with the reference's float64 result (fixture g12,
tests/golden_gen/g12_minent.py) within the per-kernel bound of DESIGN section 4: rtol 1e-4, atol 1e-5 * max|fp64|.

Segment sets: (700, 513, 300) rows with the third 3D-only at C = 5 -- several blocks with ragged tails per segment; (1, 255, 256, 257)
at C = 11 -- one row, one below / exactly / one above a block; (524588, 63) at C = 5 -- the first segment in the grid-stride regime
(2048 virtual blocks, every thread a second row, the last 300 a third)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_minent.npz")
SENTINEL = -7.25
MAXC = 64
KL, WEIGHTED, MINENT = 1, 2, 4

# (rows, in_2d) per segment
SET_A = ((700, True), (513, True), (300, False))
SET_B = ((1, True), (255, True), (256, True), (257, True))
SET_BIG = ((524588, True), (63, True))
# per segment (weighted, kl): two mixes per set
FLAGS = {SET_A: (((True, True), (False, True), (True, False)), ((False, False), (True, True), (False, False))),
         SET_B: (((True, True), (False, True), (True, False), (False, False)), ((False, True), (True, False), (True, True), (True, True))),
         SET_BIG: (((True, True), (False, True)),)}


def _lib():
    from mopa_amd import _lib
    return _lib


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _case(N, C):
    """tests/test_gpu_trainloss.py::_case: four logit matrices ~ N(0, 2), two label vectors with ~30 % of -100, class weights."""
    rng = np.random.Generator(np.random.PCG64(1000 * C + N % 9973))
    z = [torch.from_numpy(rng.standard_normal((N, C), dtype=np.float32) * 2) for _ in range(4)]
    ys = []
    for _ in range(2):
        y = rng.integers(0, C, N)
        y[rng.random(N) < 0.3] = -100
        if N == 1:
            y[:] = C - 1
        ys.append(torch.from_numpy(y))
    w = torch.from_numpy(rng.uniform(1, 3, C).astype(np.float32))
    return {"z2m": z[0], "z2x": z[1], "z3m": z[2], "z3x": z[3], "y": ys[0], "y_alt": ys[1], "w": w}


def _layout(segset):
    """-> [(n, row0_2d or -1, row0_3d)], N2, N3."""
    out, r2, r3 = [], 0, 0
    for n, in2 in segset:
        out.append((n, r2 if in2 else -1, r3))
        r2 += n if in2 else 0
        r3 += n
    return out, r2, r3


@functools.lru_cache(maxsize=2)
def _merged(segset, C):
    """Device tensors of a merged pass: the 3D network has every segment's rows, the 2D network those of the segments it takes part
    in (the 2D rows of a segment are NOT at the 3D offsets once a 3D-only segment precedes them; here it is the last).  Never written."""
    lay, N2, N3 = _layout(segset)
    c = _case(N3, C)
    rows2 = torch.cat([torch.arange(r3, r3 + n) for n, r2, r3 in lay if r2 >= 0])
    d = {"z2m": c["z2m"][rows2].contiguous().cuda(), "z2x": c["z2x"][rows2].contiguous().cuda(), "z3m": c["z3m"].cuda(), "z3x": c["z3x"].cuda(),
         "w": c["w"].cuda(), "y2": [], "y3": []}
    for n, r2, r3 in lay:
        ya, yb = c["y"][r3:r3 + n].clone(), c["y_alt"][r3:r3 + n].clone()
        if n == 1:                                                             # a one-row segment keeps its row (as _case does for N = 1)
            ya[:], yb[:] = C - 1, C - 2
        d["y2"].append(ya.cuda() if r2 >= 0 else None)
        d["y3"].append(yb.cuda())
    return d


def _heads(d, dual):
    return (d["z2m"], d["z2x"] if dual else d["z2m"], d["z3m"], d["z3x"] if dual else d["z3m"])


# ------------------------------------------------------------------------------------------------ the C ABI
def _table(descs):
    """descs: dicts with n, row0 (2), y (2), mask, conf (2), acc, flags -> the host table."""
    lib = _lib()
    t = (ctypes.c_int64 * (10 * len(descs)))()
    for s, d in enumerate(descs):
        conf = d.get("conf", (None, None))
        words = (d["n"], d["row0"][0], d["row0"][1], lib.ptr(d["y"][0]), lib.ptr(d["y"][1]), lib.ptr(d.get("mask")), lib.ptr(conf[0]),
                 lib.ptr(conf[1]), lib.ptr(d.get("acc")), d["flags"])
        t[10 * s:10 * s + 10] = [0 if v is None else int(v) for v in words]
    return t


def _rows(t):
    return 0 if t is None else t.shape[0]


def _seg_fwd(z2m, z2x, z3m, z3x, w, descs, C, scalars=None, status=None, ws=None, ws_bytes=None, S=None, ignore=-100):
    lib = _lib()
    S = len(descs) if S is None else S
    if scalars is None:
        scalars = torch.full((8 * len(descs),), SENTINEL, device="cuda")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
    if ws is None:
        ws = torch.empty(lib.query("mopa_point_losses_seg_workspace_bytes", min(max(S, 1), 8)), dtype=torch.uint8, device="cuda")
    t = _table(descs)
    lib.call("mopa_point_losses_seg_fwd", lib.ptr(z2m), lib.ptr(z2x), lib.ptr(z3m), lib.ptr(z3x), lib.ptr(w), ctypes.addressof(t), S, _rows(z2m),
             _rows(z3m), C, ignore, lib.ptr(scalars), lib.ptr(status), lib.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, lib.stream())
    return scalars, status


def _seg_bwd(net, zm, zx, other, w, descs, C, scalars, g, ignore=-100):
    """-> (dz_main, dz_xm), sentinel-filled before the call; dz_xm is dz_main on a shared head, None without an xm head."""
    lib = _lib()
    dz_main = torch.full_like(zm, SENTINEL)
    dz_xm = None if zx is None else (dz_main if zx is zm else torch.full_like(zx, SENTINEL))
    t = _table(descs)
    lib.call("mopa_point_losses_seg_bwd", net, lib.ptr(zm), lib.ptr(zx), lib.ptr(other), lib.ptr(w), ctypes.addressof(t), len(descs), _rows(zm),
             _rows(other), C, ignore, lib.ptr(scalars), lib.ptr(g), lib.ptr(dz_main), lib.ptr(dz_xm), lib.stream())
    return dz_main, dz_xm


def _slice_fwd(z2m, z2x, z3m, z3x, y2, y3, w, N, C, ignore=-100):
    """mopa_point_losses_fwd on one segment's slices -> scalars fp32[8] (ce_2d, den_2d, kl_2d, ce_3d, den_3d, kl_3d, spare)."""
    lib = _lib()
    scalars = torch.full((8,), SENTINEL, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.query("mopa_point_losses_workspace_bytes", N), dtype=torch.uint8, device="cuda")
    lib.call("mopa_point_losses_fwd", lib.ptr(z2m), lib.ptr(z2x), lib.ptr(z3m), lib.ptr(z3x), lib.ptr(y2), lib.ptr(y3), lib.ptr(w), N, C,
             ignore, lib.ptr(scalars), None, None, None, None, lib.ptr(status), lib.ptr(ws), ws.numel(), lib.stream())
    return scalars


def _slice_bwd(zm, zx, other, y, w, N, C, den, g, shared, ignore=-100):
    lib = _lib()
    like = zm if zm is not None else zx
    dz_main = torch.full_like(like, SENTINEL) if (y is not None or shared) else None
    dz_xm = dz_main if shared else (torch.full_like(like, SENTINEL) if other is not None else None)
    lib.call("mopa_point_losses_bwd", lib.ptr(zm), lib.ptr(zx), lib.ptr(other), lib.ptr(y), lib.ptr(w), N, C, ignore, lib.ptr(den),
             lib.ptr(g), lib.ptr(dz_main), lib.ptr(dz_xm), lib.stream())
    return dz_main, dz_xm


def _descs(segset, d, flags, extra=0):
    lay, _, _ = _layout(segset)
    return [{"n": n, "row0": (r2, r3), "y": (d["y2"][s], d["y3"][s]),
             "flags": (WEIGHTED if flags[s][0] else 0) | (KL if flags[s][1] else 0) | extra}
            for s, (n, r2, r3) in enumerate(lay)]


def _check_bits_of_the_slices(segset, C, dual, use_w, flags):
    d = _merged(segset, C)
    z2m, z2x, z3m, z3x = _heads(d, dual)
    w = d["w"] if use_w else None
    lay, N2, N3 = _layout(segset)
    S = len(lay)
    descs = _descs(segset, d, flags)
    sc, status = _seg_fwd(z2m, z2x, z3m, z3x, w, descs, C)
    assert status.item() == 0
    g = (torch.arange(3 * S, device="cuda", dtype=torch.float32) * 0.37 + 0.4).view(S, 3)
    got2 = _seg_bwd(0, z2m, z2x, z3m, w, descs, C, sc, g)
    got3 = _seg_bwd(1, z3m, z3x, z2m, w, descs, C, sc, g)
    for s, (n, r2, r3) in enumerate(lay):
        weighted, kl = flags[s]
        in2 = r2 >= 0
        kl = kl and in2
        ws_ = w if weighted else None
        a2m, a2x = (z2m[r2:r2 + n], z2x[r2:r2 + n]) if in2 else (None, None)
        a3m, a3x = z3m[r3:r3 + n], z3x[r3:r3 + n]
        if not dual:
            a2x, a3x = a2m, a3m                                                # the same tensor object: a shared head
        want = _slice_fwd(a2m, a2x if kl else None, a3m, a3x if kl else None, d["y2"][s], d["y3"][s], ws_, n, C)
        mine = sc[8 * s:8 * s + 8]
        print(segset, C, dual, use_w, flags[s], s, mine.tolist(), want.tolist())
        for k in range(2):                                                     # (ce, den, kl) per network; ent is absent: untouched
            assert _same_bits(mine[4 * k:4 * k + 3], want[3 * k:3 * k + 3]), (s, k)
            assert mine[4 * k + 3].item() == SENTINEL
        assert torch.isfinite(want[3:5]).all() and (not in2 or torch.isfinite(want[0:2]).all())
        # gradient rows of this segment
        for k, (zm, zx, other, y, row, got) in enumerate(((a2m, a2x, a3m, d["y2"][s], r2, got2), (a3m, a3x, a2m, d["y3"][s], r3, got3))):
            if zm is None:
                continue
            den = want[3 * k + 1:3 * k + 2]
            dm, dx = _slice_bwd(zm, zx if kl else None, other if kl else None, y, ws_, n, C, den, g[s, :2].contiguous(), shared=kl and not dual)
            got_main, got_xm = got[0][row:row + n], got[1][row:row + n]
            assert _same_bits(got_main, dm), (s, k, "main")
            if dual:
                if kl:
                    assert _same_bits(got_xm, dx), (s, k, "xm")
                else:
                    assert (_bits(got_xm) == 0).all(), (s, k, "xm rows of a segment without KL")
    assert not (got2[0] == SENTINEL).any() and not (got3[0] == SENTINEL).any()          # every row is written
    assert not (got2[1] == SENTINEL).any() and not (got3[1] == SENTINEL).any()


@pytest.mark.parametrize("dual", (True, False))
@pytest.mark.parametrize("segset,C", ((SET_A, 5), (SET_B, 11)))
def test_scalars_and_gradient_rows_have_the_bits_of_the_slice_calls(segset, C, dual):
    for use_w in (True, False):
        for flags in FLAGS[segset]:
            _check_bits_of_the_slices(segset, C, dual, use_w, flags)


@pytest.mark.parametrize("dual", (True, False))
def test_grid_stride_segment_has_the_bits_of_the_slice_calls(dual):
    _check_bits_of_the_slices(SET_BIG, 5, dual, True, FLAGS[SET_BIG][0])


# ------------------------------------------------------------------------------------------------ the Python API
def _leaves(segset, C, dual):
    d = _merged(segset, C)
    names = ("z2m", "z2x", "z3m", "z3x") if dual else ("z2m", "z3m")
    L = {k: d[k].clone().requires_grad_(True) for k in names}
    p2, p3 = {"seg_logit": L["z2m"]}, {"seg_logit": L["z3m"]}
    if dual:
        p2["seg_logit2"], p3["seg_logit2"] = L["z2x"], L["z3x"]
    return d, L, p2, p3


def _segments(segset, d, flags, **kw):
    from mopa_amd.trainloss import Segment
    return [Segment(n, label_2d=d["y2"][s], label_3d=d["y3"][s], weighted=flags[s][0], kl=flags[s][1], in_2d=in2, **kw)
            for s, (n, in2) in enumerate(segset)]


def _sliced_recipe(segset, C, dual, flags, w, **kw):
    """point_losses per segment on slices of the merged leaves -> (leaves, per-segment PointLosses)."""
    from mopa_amd.trainloss import point_losses
    d, L, p2, p3 = _leaves(segset, C, dual)
    lay, _, _ = _layout(segset)
    res = []
    for s, (n, r2, r3) in enumerate(lay):
        q2 = None if r2 < 0 else {k: v[r2:r2 + n] for k, v in p2.items()}
        q3 = {k: v[r3:r3 + n] for k, v in p3.items()}
        res.append(point_losses(q2, q3, label_2d=d["y2"][s], label_3d=d["y3"][s], weight=w if flags[s][0] else None, kl=flags[s][1], **kw))
    return L, res


def _sum(terms):
    terms = [t for t in terms if t is not None]
    return sum(terms[1:], terms[0])


@pytest.mark.parametrize("dual", (True, False))
@pytest.mark.parametrize("segset,C", ((SET_A, 5), (SET_B, 11)))
def test_point_losses_merged_equals_the_sliced_recipe(segset, C, dual):
    from mopa_amd.trainloss import point_losses_merged
    for flags in FLAGS[segset]:
        d, L, p2, p3 = _leaves(segset, C, dual)
        res = point_losses_merged(p2, p3, _segments(segset, d, flags), weight=d["w"])
        lam = [0.1 + 0.05 * s for s in range(len(segset))]
        _sum([r.ce_2d for r in res.segments] + [a * r.kl_2d for a, r in zip(lam, res.segments) if r.kl_2d is not None]).backward()
        _sum([r.ce_3d for r in res.segments] + [a * r.kl_3d for a, r in zip(lam, res.segments) if r.kl_3d is not None]).backward()
        R, ref = _sliced_recipe(segset, C, dual, flags, d["w"])
        _sum([r.ce_2d for r in ref] + [a * r.kl_2d for a, r in zip(lam, ref) if r.kl_2d is not None]).backward()
        _sum([r.ce_3d for r in ref] + [a * r.kl_3d for a, r in zip(lam, ref) if r.kl_3d is not None]).backward()
        for s, (got, want) in enumerate(zip(res.segments, ref)):
            for name in ("ce_2d", "kl_2d", "ce_3d", "kl_3d"):
                a, b = getattr(got, name), getattr(want, name)
                assert (a is None) == (b is None), (s, name)
                if a is not None:
                    assert a.dim() == 0 and a.requires_grad and torch.equal(a, b) and _same_bits(a, b), (s, name)
            assert got.ent_2d is None and got.ent_3d is None and got.acc is None
        for k in L:
            if R[k].grad is None:                                              # no slice has a term for this head
                assert L[k].grad is None or (L[k].grad == 0).all(), k
            else:
                assert torch.equal(L[k].grad, R[k].grad), k
        assert res.status.item() == 0


@pytest.mark.parametrize("dual", (True, False))
def test_one_segment_equals_point_losses(dual):
    from mopa_amd.models.metric import SegIoU
    from mopa_amd.trainloss import Segment, point_losses, point_losses_merged
    N, C = 4099, 10
    c = _case(N, C)
    y, w = c["y"].cuda(), c["w"].cuda()
    mask = (c["y_alt"] != -100).cuda()

    def leaves():
        names = ("z2m", "z2x", "z3m", "z3x") if dual else ("z2m", "z3m")
        L = {k: c[k].cuda().requires_grad_(True) for k in names}
        p2, p3 = {"seg_logit": L["z2m"]}, {"seg_logit": L["z3m"]}
        if dual:
            p2["seg_logit2"], p3["seg_logit2"] = L["z2x"], L["z3x"]
        return L, p2, p3

    L, p2, p3 = leaves()
    m2, m3 = SegIoU(C), SegIoU(C)
    res = point_losses_merged(p2, p3, [Segment(N, label=y, metric_2d=m2, metric_3d=m3, acc_mask=mask)], weight=w)
    got = res.segments[0]
    (got.ce_2d + 0.1 * got.kl_2d).backward()
    (got.ce_3d + 0.1 * got.kl_3d).backward()
    R, q2, q3 = leaves()
    u2, u3 = SegIoU(C), SegIoU(C)
    want = point_losses(q2, q3, label=y, weight=w, metric_2d=u2, metric_3d=u3, acc_mask=mask)
    (want.ce_2d + 0.1 * want.kl_2d).backward()
    (want.ce_3d + 0.1 * want.kl_3d).backward()
    for name in ("ce_2d", "kl_2d", "ce_3d", "kl_3d"):
        assert torch.equal(getattr(got, name), getattr(want, name)) and _same_bits(getattr(got, name), getattr(want, name)), name
    for k in L:
        assert torch.equal(L[k].grad, R[k].grad) and _same_bits(L[k].grad, R[k].grad), k
    assert torch.equal(m2.mat, u2.mat) and torch.equal(m3.mat, u3.mat) and int(m3.mat.sum()) == int((y != -100).sum())
    assert got.acc.dtype == torch.int64 and torch.equal(got.acc, want.acc) and int(got.acc[1]) == int(mask.sum())
    assert torch.equal(res.status, want.status) and res.status.dtype == torch.int32 and res.status.item() == 0


# ------------------------------------------------------------------------------------------------ integers
def _np_conf(z, y, C):
    mat = np.zeros((C, C), np.int64)
    z, y = z.cpu().numpy(), y.cpu().numpy()
    keep = y != -100
    np.add.at(mat, (y[keep], np.argmax(z, 1)[keep]), 1)
    return torch.from_numpy(mat)


def test_confusion_matrices_and_accuracy_per_segment():
    from mopa_amd.models.metric import SegIoU
    from mopa_amd.trainloss import Segment, point_losses_merged
    segset, C = SET_A, 5
    d = _merged(segset, C)
    lay, _, _ = _layout(segset)
    metrics = [(SegIoU(C), SegIoU(C)), (None, SegIoU(C)), (None, None)]          # the last segment has no metric at all
    rng = np.random.Generator(np.random.PCG64(5))
    masks = [torch.from_numpy(rng.random(n) < 0.2).cuda() for n, _, _ in lay]
    segs = [Segment(n, label_2d=d["y2"][s], label_3d=d["y3"][s], in_2d=r2 >= 0, metric_2d=metrics[s][0], metric_3d=metrics[s][1],
                    acc_mask=masks[s] if s != 1 else None) for s, (n, r2, r3) in enumerate(lay)]
    p2, p3 = {"seg_logit": d["z2m"]}, {"seg_logit": d["z3m"]}
    for rep in (1, 2):                                                           # SegIoU accumulates over calls
        res = point_losses_merged(p2, p3, segs)
        for s, (n, r2, r3) in enumerate(lay):
            z3, y3 = d["z3m"][r3:r3 + n], d["y3"][s]
            if metrics[s][0] is not None:
                assert torch.equal(metrics[s][0].mat.cpu(), rep * _np_conf(d["z2m"][r2:r2 + n], d["y2"][s], C)), s
            if metrics[s][1] is not None:
                assert torch.equal(metrics[s][1].mat.cpu(), rep * _np_conf(z3, y3, C)), s
            if s == 1:
                assert res.segments[s].acc is None
            else:
                m = masks[s].cpu().numpy()
                hit = int(((np.argmax(z3.cpu().numpy(), 1) == y3.cpu().numpy()) & m).sum())
                assert res.segments[s].acc.tolist() == [hit, int(m.sum())] and 0 < hit < int(m.sum())
    # through the C ABI the matrices and counts are ADDED to, per segment, and a segment without matrices adds nothing
    conf = torch.full((3, 2, C, C), 3, dtype=torch.int64, device="cuda")
    acc = torch.full((3, 2), 10, dtype=torch.int64, device="cuda")
    descs = _descs(segset, d, ((True, True),) * 3)
    descs[0].update(conf=(conf[0, 0], conf[0, 1]), mask=masks[0].view(torch.uint8), acc=acc[0])
    descs[1].update(conf=(None, conf[1, 1]))
    _seg_fwd(d["z2m"], d["z2m"], d["z3m"], d["z3m"], None, descs, C)
    assert torch.equal(conf[0, 0].cpu() - 3, _np_conf(d["z2m"][:700], d["y2"][0], C)) and torch.equal(conf[0, 1].cpu() - 3, _np_conf(d["z3m"][:700], d["y3"][0], C))
    assert torch.equal(conf[1, 1].cpu() - 3, _np_conf(d["z3m"][700:1213], d["y3"][1], C))
    assert (conf[1, 0] == 3).all() and (conf[2] == 3).all() and (acc[1:] == 10).all() and int(acc[0, 1]) == 10 + int(masks[0].sum())


# ------------------------------------------------------------------------------------------------ degenerate forms
def test_zero_row_segment_gives_nan_terms_and_leaves_the_others_alone():
    from mopa_amd.trainloss import Segment, point_losses_merged
    segset, C = SET_A, 5
    flags = FLAGS[segset][0]
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    d, L, p2, p3 = _leaves(segset, C, True)
    base = point_losses_merged(p2, p3, _segments(segset, d, flags), weight=d["w"])
    _sum([t for r in base.segments for t in (r.ce_3d, r.kl_3d)]).backward()
    d, M, q2, q3 = _leaves(segset, C, True)
    segs = _segments(segset, d, flags)
    segs.insert(1, Segment(0, label=empty))
    res = point_losses_merged(q2, q3, segs, weight=d["w"])
    z = res.segments[1]
    for t in (z.ce_2d, z.kl_2d, z.ce_3d, z.kl_3d):
        assert t.dim() == 0 and torch.isnan(t) and t.requires_grad
    others = [res.segments[0]] + res.segments[2:]
    for got, want in zip(others, base.segments):
        for name in ("ce_2d", "kl_2d", "ce_3d", "kl_3d"):
            a, b = getattr(got, name), getattr(want, name)
            assert (a is None) == (b is None) and (a is None or _same_bits(a, b)), name
    _sum([t for r in others for t in (r.ce_3d, r.kl_3d)]).backward()             # the zero-row segment's terms unused
    for k in ("z3m", "z3x"):
        assert _same_bits(M[k].grad, L[k].grad), k
    # through the C ABI: NaN (0 / 0 and 0 * inf), normaliser 0
    dd = _merged(segset, C)
    descs = _descs(segset, dd, flags)
    descs.insert(1, {"n": 0, "row0": (700, 700), "y": (dd["y2"][0], dd["y3"][0]), "flags": KL | MINENT})
    sc, _ = _seg_fwd(dd["z2m"], dd["z2x"], dd["z3m"], dd["z3x"], dd["w"], descs, C)
    got = sc[8:16].cpu()
    assert torch.isnan(got[[0, 2, 3, 4, 6, 7]]).all() and got[1] == 0 and got[5] == 0


def test_all_labels_of_one_segment_ignored():
    from mopa_amd.trainloss import point_losses_merged
    segset, C = SET_A, 5
    flags = FLAGS[segset][0]
    d, L, p2, p3 = _leaves(segset, C, False)
    base = point_losses_merged(p2, p3, _segments(segset, d, flags), weight=d["w"])
    segs = _segments(segset, d, flags)
    segs[1].label_2d = torch.full_like(d["y2"][1], -100)
    res = point_losses_merged(p2, p3, segs, weight=d["w"])
    assert torch.isnan(res.segments[1].ce_2d) and res.status.item() == 0
    for s, (got, want) in enumerate(zip(res.segments, base.segments)):
        for name in ("ce_2d", "kl_2d", "ce_3d", "kl_3d"):
            a, b = getattr(got, name), getattr(want, name)
            if (s, name) != (1, "ce_2d") and a is not None:
                assert torch.isfinite(a) and _same_bits(a, b), (s, name)
    _sum([r.ce_2d + 0.1 * r.kl_2d for r in res.segments if r.kl_2d is not None]).backward()
    g = L["z2m"].grad
    assert torch.isfinite(g).all() and (g[:700] != 0).any() and (g[700:] != 0).any()   # the KL part of segment 1 is still there


def test_out_of_range_label_sets_status_and_raises_only_under_validation(monkeypatch):
    from mopa_amd.common.utils import loss as single
    from mopa_amd.trainloss import point_losses_merged
    segset, C = SET_A, 5
    flags = FLAGS[segset][0]
    d = _merged(segset, C)
    p2, p3 = {"seg_logit": d["z2m"]}, {"seg_logit": d["z3m"]}
    clean = _segments(segset, d, flags)
    bad = _segments(segset, d, flags)
    y = d["y3"][2].clone()
    y[7] = C
    bad[2].label_3d = y
    ign = _segments(segset, d, flags)
    y = y.clone()
    y[7] = -100
    ign[2].label_3d = y
    r_bad, r_ign = point_losses_merged(p2, p3, bad, weight=d["w"]), point_losses_merged(p2, p3, ign, weight=d["w"])
    assert r_bad.status.item() == 1 and r_ign.status.item() == 0                 # flagged, not raised; dropped like an ignored row
    assert _same_bits(r_bad.segments[2].ce_3d, r_ign.segments[2].ce_3d)
    assert point_losses_merged(p2, p3, clean, weight=d["w"]).status.item() == 0
    monkeypatch.setattr(single, "VALIDATE_LABELS", True)
    with pytest.raises(IndexError):
        point_losses_merged(p2, p3, bad, weight=d["w"])
    assert point_losses_merged(p2, p3, clean, weight=d["w"]).status.item() == 0


def test_unused_terms_contribute_exact_zeros():
    from mopa_amd.trainloss import point_losses_merged
    segset, C = SET_A, 5
    flags = ((True, True),) * 3
    d, L, p2, p3 = _leaves(segset, C, True)
    res = point_losses_merged(p2, p3, _segments(segset, d, flags, minent=True), weight=d["w"])
    res.segments[1].ce_3d.backward()                                             # every other upstream gradient of the 3D node is None
    g = L["z3m"].grad
    assert (g[:700] == 0).all() and (g[1213:] == 0).all() and (g[700:1213] != 0).any() and torch.isfinite(g).all()
    assert (L["z3x"].grad == 0).all()
    assert L["z2m"].grad is None and L["z2x"].grad is None
    want = _slice_bwd(d["z3m"][700:1213], None, None, d["y3"][1], d["w"], 513, C, _slice_fwd(None, None, d["z3m"][700:1213], None, None,
                      d["y3"][1], d["w"], 513, C)[4:5], torch.tensor((1.0, 0.0), device="cuda"), shared=False)[0]
    assert torch.equal(g[700:1213], want)                                        # + 0 of the entropy part: the value is unchanged


# ------------------------------------------------------------------------------------------------ MinEnt
@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def _close(got, ref64, what):
    """DESIGN section 4, per kernel: |got - ref| <= 1e-4 |ref| + 1e-5 max|ref|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    bound = 1e-4 * np.abs(ref) + 1e-5 * np.abs(ref).max()
    print(what, "worst |err| / bound", float((err / bound).max()))
    assert (err <= bound).all(), f"{what}: worst |err| {err.max():.3e}, {int((err > bound).sum())} outside the bound"


@pytest.mark.parametrize("k", range(4))
def test_minent_against_the_reference_in_float64(k):
    from mopa_amd.trainloss import Segment, point_losses_merged
    G = _golden()
    N, C = (int(v) for v in G["cases"][k])
    assert (N, C) == ((63, 2), (257, 5), (1000, 11), (4099, 10))[k]
    z = torch.from_numpy(G[f"c{k}_z"])
    assert z[0, 0] == 120 and (z[0, 1:] == 0).all()                              # the saturated row
    for net in (0, 1):
        leaf = z.cuda().requires_grad_(True)
        preds = [None, None]
        preds[net] = {"seg_logit": leaf}
        res = point_losses_merged(preds[0], preds[1], [Segment(N, minent=True)])
        r = res.segments[0]
        ent = (r.ent_2d, r.ent_3d)[net]
        assert (r.ent_3d, r.ent_2d)[net] is None and r.ce_2d is None and r.kl_3d is None and ent.dim() == 0
        _close(ent.item(), G[f"c{k}_loss64"], f"minent loss {N, C} net {net}")
        ent.backward()
        _close(leaf.grad.cpu().numpy(), G[f"c{k}_grad64"], f"minent gradient {N, C} net {net}")
        # the reference's own fp32 result sits far inside the same bound
        _close(G[f"c{k}_grad32"], G[f"c{k}_grad64"], f"reference fp32 gradient {N, C}")


def test_minent_in_a_mixed_segment_set_leaves_the_other_segments_bits():
    from mopa_amd.trainloss import Segment, point_losses_merged
    G = _golden()
    C = 5
    zg = torch.from_numpy(G["c1_z"])                                              # (257, 5): the middle segment
    segset = ((700, True), (257, True), (300, False))
    lay, N2, N3 = _layout(segset)
    c = _case(N3, C)
    runs = {}
    for minent in (False, True):
        for dual in (True, False):
            L = {}
            for name, rows in (("z2m", N2), ("z2x", N2), ("z3m", N3), ("z3x", N3)):
                if not dual and name in ("z2x", "z3x"):
                    continue
                t = c[name][:rows].clone()
                if name in ("z2m", "z3m"):
                    t[700:957] = zg
                L[name] = t.cuda().requires_grad_(True)
            p2, p3 = {"seg_logit": L["z2m"]}, {"seg_logit": L["z3m"]}
            if dual:
                p2["seg_logit2"], p3["seg_logit2"] = L["z2x"], L["z3x"]
            ys = [c["y"][r3:r3 + n].cuda() for n, r2, r3 in lay]
            segs = [Segment(700, label=ys[0]), Segment(257, label=ys[1], minent=minent), Segment(300, label_3d=ys[2], in_2d=False, kl=False)]
            res = point_losses_merged(p2, p3, segs, weight=c["w"].cuda())
            lam = 0.25
            for which in ("2d", "3d"):
                terms = [getattr(r, "ce_" + which) for r in res.segments if getattr(r, "ce_" + which) is not None]
                terms += [0.1 * getattr(r, "kl_" + which) for r in res.segments if getattr(r, "kl_" + which) is not None]
                if minent:
                    terms.append(lam * getattr(res.segments[1], "ent_" + which))
                _sum(terms).backward()
            runs[minent, dual] = (res, L)
    for dual in (True, False):
        (r0, L0), (r1, L1) = runs[False, dual], runs[True, dual]
        for s in range(3):
            for name in ("ce_2d", "kl_2d", "ce_3d", "kl_3d"):
                a, b = getattr(r0.segments[s], name), getattr(r1.segments[s], name)
                assert (a is None) == (b is None) and (a is None or _same_bits(a, b)), (s, name)
            assert r0.segments[s].ent_2d is None and r0.segments[s].ent_3d is None
            assert (r1.segments[s].ent_2d is None) == (s != 1) and (r1.segments[s].ent_3d is None) == (s != 1)
        for name in ("ent_2d", "ent_3d"):
            _close(getattr(r1.segments[1], name).item(), G["c1_loss64"], name + " inside a mixed set")
        for k in L0:
            a, b = L0[k].grad, L1[k].grad
            assert _same_bits(a[:700], b[:700]) and _same_bits(a[957:], b[957:]), k   # segments without MinEnt: the same bits
            if k in ("z2m", "z3m"):
                # the middle segment's main head: the CE / KL rows plus lam * the entropy gradient (a sum of fp32 parts: rtol
                # 1e-4 and atol 1e-5 * max|entropy gradient| on the DIFFERENCE, plus one rounding of the sum)
                diff = (b[700:957].double() - a[700:957].double()).cpu().numpy()
                ref = lam * G["c1_grad64"]
                err = np.abs(diff - ref)
                bound = 1e-4 * np.abs(ref) + 1e-5 * np.abs(ref).max() + 2.0 ** -23 * np.abs(b[700:957].cpu().numpy())
                assert (err <= bound).all(), (k, float(err.max()))
            else:
                assert _same_bits(a, b), k


# ------------------------------------------------------------------------------------------------ structure
class _Recorder:
    """trainloss.call with the entry-point names (and the stream argument) written down."""

    def __init__(self, monkeypatch, module):
        self.names, self.streams, inner = [], [], module.call

        def call(name, *args):
            self.names.append(name)
            self.streams.append(args[-1])
            return inner(name, *args)
        monkeypatch.setattr(module, "call", call)


@pytest.mark.parametrize("dual", (True, False))
def test_launch_count(dual, monkeypatch):
    from mopa_amd import trainloss
    from mopa_amd.common.utils import loss as single
    from mopa_amd.models.metric import SegIoU
    segset, C = SET_A, 5
    rec = _Recorder(monkeypatch, trainloss)
    other = _Recorder(monkeypatch, single)
    d, L, p2, p3 = _leaves(segset, C, dual)
    segs = _segments(segset, d, FLAGS[segset][0], minent=True, metric_3d=SegIoU(C))
    res = trainloss.point_losses_merged(p2, p3, segs, weight=d["w"])
    assert rec.names == ["mopa_point_losses_seg_fwd"]
    _sum([t for r in res.segments for t in (r.ce_2d, r.kl_2d, r.ent_2d)]).backward()
    assert rec.names == ["mopa_point_losses_seg_fwd", "mopa_point_losses_seg_bwd"]
    _sum([t for r in res.segments for t in (r.ce_3d, r.kl_3d, r.ent_3d)]).backward()
    assert rec.names == ["mopa_point_losses_seg_fwd", "mopa_point_losses_seg_bwd", "mopa_point_losses_seg_bwd"]
    assert other.names == []                                           # no mopa_wce_* / mopa_softmax_kl_*
    assert all(g.grad is not None and g.grad.shape == g.shape for g in L.values())


@pytest.mark.parametrize("dual_head", (True, False))
def test_dual_stream_runs_the_3d_backward_on_the_side_stream(dual_head, monkeypatch):
    from mopa_amd import trainloss
    from mopa_amd.step import DualStream
    segset, C = SET_A, 5
    runs = {}
    for use_dual in (False, True):
        dual = DualStream("cuda") if use_dual else None
        rec = _Recorder(monkeypatch, trainloss)
        d, L, p2, p3 = _leaves(segset, C, dual_head)
        main = torch.cuda.current_stream().cuda_stream
        res = trainloss.point_losses_merged(p2, p3, _segments(segset, d, FLAGS[segset][0], minent=True), weight=d["w"], dual=dual)
        seen = {}
        for k in L:
            L[k].register_hook(lambda g, k=k: seen.__setitem__(k, torch.cuda.current_stream().cuda_stream))
        loss2 = _sum([t for r in res.segments for t in (r.ce_2d, r.kl_2d, r.ent_2d)])
        loss3 = _sum([t for r in res.segments for t in (r.ce_3d, r.kl_3d, r.ent_3d)])
        loss2.backward()
        if use_dual:
            dual.backward_on_side(loss3)
            dual.join()
        else:
            loss3.backward()
        assert torch.cuda.current_stream().cuda_stream == main
        side = dual.side.cuda_stream if use_dual else main
        assert use_dual == (side != main)
        assert rec.names == ["mopa_point_losses_seg_fwd", "mopa_point_losses_seg_bwd", "mopa_point_losses_seg_bwd"]
        assert rec.streams == [main, main, side]
        for k in L:
            assert seen[k] == (side if k.startswith("z3") else main), k
        runs[use_dual] = [t for r in res.segments for t in (r.ce_2d, r.kl_2d, r.ent_2d, r.ce_3d, r.kl_3d, r.ent_3d) if t is not None]
        runs[use_dual] += [L[k].grad for k in sorted(L)]
        monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(runs[False]) == len(runs[True])
    for a, b in zip(runs[False], runs[True]):
        assert torch.equal(a, b) and _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_calls_write_nothing():
    lib = _lib()
    n, C = 300, 5
    rng = torch.Generator().manual_seed(3)

    def outputs(C, S=2):
        return {"scalars": torch.full((8 * 9,), SENTINEL, device="cuda"), "conf": torch.full((2, C, C), 77, dtype=torch.int64, device="cuda"),
                "acc": torch.full((2,), 77, dtype=torch.int64, device="cuda"), "status": torch.full((1,), 4, dtype=torch.int32, device="cuda"),
                "dz": torch.full((2, 2 * n, C), SENTINEL, device="cuda")}

    def untouched(o):
        torch.cuda.synchronize()
        return bool((o["scalars"] == SENTINEL).all() and (o["conf"] == 77).all() and (o["acc"] == 77).all() and (o["status"] == 4).all()
                    and (o["dz"] == SENTINEL).all())

    def inputs(C):
        z = torch.randn(2, 2 * n, C, generator=rng).cuda()
        y = torch.zeros(n, dtype=torch.int64, device="cuda")
        mask = torch.ones(n, dtype=torch.uint8, device="cuda")
        return z, y, mask

    def descs(o, y, mask, S=2):
        return [{"n": n, "row0": (n * s, n * s), "y": (y, y), "mask": mask, "conf": (o["conf"][0], o["conf"][1]), "acc": o["acc"], "flags": KL | MINENT}
                for s in range(S)]

    need = lib.query("mopa_point_losses_seg_workspace_bytes", 2)
    assert need >= 2 * 8 * 2048 * 8
    ws = torch.empty(lib.query("mopa_point_losses_seg_workspace_bytes", 8), dtype=torch.uint8, device="cuda")
    arg, wsp = r"mopa_point_losses_seg_fwd failed with code -1$", r"mopa_point_losses_seg_fwd failed with code -2$"

    z, y, mask = inputs(MAXC + 1)                                                  # C > 64
    o = outputs(MAXC + 1)
    with pytest.raises(RuntimeError, match=arg):
        _seg_fwd(z[0], z[0], z[1], z[1], None, descs(o, y, mask), MAXC + 1, o["scalars"], o["status"], ws)
    assert untouched(o)
    z, y, mask = inputs(C)
    o = outputs(C)
    with pytest.raises(RuntimeError, match=wsp):                                   # a short workspace
        _seg_fwd(z[0], z[0], z[1], z[1], None, descs(o, y, mask), C, o["scalars"], o["status"], ws, ws_bytes=need - 1)
    assert untouched(o)
    nine = [{"n": 66 if s < 8 else 72, "row0": (66 * s, 66 * s), "y": (None, None), "flags": KL} for s in range(9)]
    with pytest.raises(RuntimeError, match=arg):                                   # S > 8
        _seg_fwd(z[0], z[0], z[1], z[1], None, nine, C, o["scalars"], o["status"], ws)
    assert untouched(o)
    with pytest.raises(RuntimeError, match=arg):                                   # a network's row0 given without its logits
        _seg_fwd(None, None, z[1], z[1], None, descs(o, y, mask), C, o["scalars"], o["status"], ws)
    assert untouched(o)
    dd = descs(o, y, mask)
    dd[1]["y"] = (None, y)                                                         # matrices without labels
    with pytest.raises(RuntimeError, match=arg):
        _seg_fwd(z[0], z[0], z[1], z[1], None, dd, C, o["scalars"], o["status"], ws)
    assert untouched(o)
    dd = descs(o, y, mask)
    dd[1]["row0"] = (n + 1, n)                                                     # rows that are not the concatenation of the segments
    with pytest.raises(RuntimeError, match=arg):
        _seg_fwd(z[0], z[0], z[1], z[1], None, dd, C, o["scalars"], o["status"], ws)
    assert untouched(o)
    one = torch.randn(2, 2 * n, 1, generator=rng).cuda()                           # minent with one class
    o1 = outputs(1)
    with pytest.raises(RuntimeError, match=arg):
        _seg_fwd(one[0], one[0], one[1], one[1], None, descs(o1, y, mask), 1, o1["scalars"], o1["status"], ws)
    assert untouched(o1)
    _seg_fwd(z[0], z[0], z[1], z[1], None, descs(o, y, mask), C, o["scalars"], o["status"], ws, ws_bytes=need)    # the exact size is taken
    torch.cuda.synchronize()
    assert not untouched(o) and int(o["acc"][1]) == 77 + 2 * n and (o["scalars"][:16] != SENTINEL).all() and (o["scalars"][16:] == SENTINEL).all()

    # backward
    o = outputs(C)
    sc, g = torch.ones(16, device="cuda"), torch.ones(6, device="cuda")
    dd = [{"n": n, "row0": (n * s, n * s), "y": (y, y), "flags": KL} for s in range(2)]
    t = _table(dd)

    def bwd(C, z_xm, dz_xm, S=2, rows=2 * n, net=0):
        lib.call("mopa_point_losses_seg_bwd", net, lib.ptr(z[0]), z_xm, lib.ptr(z[1]), None, ctypes.addressof(t), S, rows, 2 * n, C, -100,
                 lib.ptr(sc), lib.ptr(g), lib.ptr(o["dz"][0]), dz_xm, lib.stream())

    for args in ((C, lib.ptr(z[0]), lib.ptr(o["dz"][1])),          # a shared head with two gradient buffers
                 (C, lib.ptr(z[1]), lib.ptr(o["dz"][0])),          # two heads with one gradient buffer
                 (C, lib.ptr(z[1]), None),                         # an xm head without its gradient buffer
                 (MAXC + 1, lib.ptr(z[0]), lib.ptr(o["dz"][0])),
                 (C, lib.ptr(z[0]), lib.ptr(o["dz"][0]), 9),       # S > 8
                 (C, lib.ptr(z[0]), lib.ptr(o["dz"][0]), 2, 2 * n - 1),   # rows that do not add up
                 (C, lib.ptr(z[0]), lib.ptr(o["dz"][0]), 2, 2 * n, 2)):   # no such network
        with pytest.raises(RuntimeError, match=r"mopa_point_losses_seg_bwd failed with code -1$"):
            bwd(*args)
        assert untouched(o)
    bwd(C, lib.ptr(z[0]), lib.ptr(o["dz"][0]))
    torch.cuda.synchronize()
    assert (o["dz"][0] != SENTINEL).all() and (o["dz"][1] == SENTINEL).all()


def test_one_call_workspace_is_one_segments():
    """mopa_point_losses_fwd runs the segment kernels over one segment: its workspace is that segment's, whatever N."""
    lib = _lib()
    one = lib.query("mopa_point_losses_seg_workspace_bytes", 1)
    for N in (1, 524588):
        assert lib.query("mopa_point_losses_workspace_bytes", N) == one
