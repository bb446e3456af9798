"""The linear heads through the C ABI against float64: mopa_output_layer_heads_{fwd,bwd} (csrc/rows.hip, the point heads of both
networks) and mopa_pixel_head_{fwd,bwd} (csrc/ops2d.hip, the full-image head), at the widths, class counts and point counts where
their kernels change path -- idle lanes (M/4 not a power of two), the <8> / <HEAD_MAXNC> weight-gradient kernels on both sides of
8 classes, the largest class count of every width, one and two weight-gradient blocks, the four-points-in-flight loop with and
without a remainder, channel slices of wider buffers, empty and crowded rows, null gradients, accumulation -- and the class limit:
one (M, NC) set for forward and backward, the first count outside it refused before anything is launched.

Inputs are fp32 from fixed seeds on the CPU; the reference is the same numbers in float64 with plain torch.  Tolerances are
derived: an n-term fp32 sum in any order has |error| <= n * 2^-24 * sum|terms|; a factor 2 covers the fma / bias / final
roundings.  `n` is named beside every assertion and sum|terms| is computed in float64 from the same inputs."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = -12345.678   # pre-fill of every output buffer: what a kernel must not touch keeps these bits


# ---------------------------------------------------------------------------------------------------------------- the class limit
def _lanes(M):
    q = 1
    while q < M // 4:
        q *= 2
    return q


def point_limit(M):
    """This file's own statement of mopa_heads_supported: 16 classes by registers, and (256 / lanes) * NC * (M + 1) floats of LDS
    staging within 64 KiB (test_limits_are_the_predicates holds it against the library)."""
    return min(16, 65536 // ((256 // _lanes(M)) * (M + 1) * 4))


def pixel_limit(M):
    """mopa_pixel_head_supported: additionally one lane (M / 4 of them) per class."""
    return min(16, M // 4, 65536 // ((256 // (M // 4)) * (M + 1) * 4))


POINT_M = (4, 8, 12, 16, 20, 48, 64)
PIXEL_M = (16, 64, 128, 256)
POINT_CASES = [(M, nc) for M in POINT_M for nc in sorted({1, 5, 8, 9, 11, point_limit(M)}) if nc <= point_limit(M)]
# (the full-image head takes at most M / 4 = 4 classes at M = 16: the counts above its limit are left out, never passed)
PIXEL_CASES = [(M, nc) for M in PIXEL_M for nc in sorted({1, 5, 11, pixel_limit(M)}) if nc <= pixel_limit(M)]


def _lib():
    from mopa_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _within(got, ref, bound, what):
    """|got - ref| <= bound elementwise (float64 on the host); a NaN anywhere fails."""
    got, ref, bound = (np.asarray(x, dtype=np.float64) for x in (got, ref, bound))
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.nan_to_num(err, nan=np.inf), -1.0)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.size} outside the bound; worst at {i}: got {got[i]!r}, want {ref[i]!r}, "
                             f"|err| {err[i]:.3e} > {bound[i]:.3e}")


def test_limits_are_the_predicates():
    """The (M, NC) sets of the two heads, as the summary states them, are what the library answers -- and forward and backward
    share the answer because both launchers ask it (the rejection tests below)."""
    q = _lib().query
    for M in range(0, 80):
        for nc in range(0, 40):
            want = M > 0 and M % 4 == 0 and M <= 64 and 0 < nc <= point_limit(M)
            assert bool(q("mopa_heads_supported", M, nc)) == want, (M, nc)
    for M in list(range(0, 80)) + [96, 128, 192, 256, 260, 512, 1024]:
        for nc in range(0, 40):
            mq = M // 4
            want = M > 0 and M % 4 == 0 and (mq & (mq - 1)) == 0 and mq <= 64 and 0 < nc <= pixel_limit(M)
            assert bool(q("mopa_pixel_head_supported", M, nc)) == want, (M, nc)
    assert [point_limit(M) for M in (4, 8, 12, 16, 20, 32, 48, 64)] == [12, 14, 16, 15, 16, 15, 16, 15]
    assert [pixel_limit(M) for M in (16, 32, 64, 128, 256)] == [4, 8, 15, 15, 15]


# ---------------------------------------------------------------------------------------------------------------- point heads
def _point_rows(rng, N):
    """point_row (N,) int32 into A > N rows: 3-5 points on one row (where N allows), rows without a point, random otherwise."""
    A = N + 9
    pr = rng.integers(0, A, N)
    if N >= 12:
        pr[[0, N // 2, N - 1]] = 3                       # three points far apart on row 3
        pr[1:6] = 5                                      # five neighbours on row 5
        pr[N - 5:N - 1] = A - 1                          # four on the last row
        pr[pr == 0] = 1                                  # row 0 and row 7 stay empty
        pr[pr == 7] = 8
    return pr.astype(np.int32), A


def _csr(point_row, A):
    lib = _lib()
    N = len(point_row)
    pr = _dev(point_row)
    row_start = torch.full((A + 2,), -7, dtype=torch.int32, device="cuda")
    row_points = torch.full((N + 1,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(lib.query("mopa_points_csr_workspace_bytes", A), 256), dtype=torch.uint8, device="cuda")
    lib.call("mopa_points_csr", lib.ptr(pr), N, A, lib.ptr(row_start), lib.ptr(row_points), lib.ptr(ws), ws.numel(), lib.stream())
    order = np.argsort(point_row, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(point_row, minlength=A))])
    assert np.array_equal(row_start.cpu().numpy()[:A + 1], start) and row_start[A + 1].item() == -7
    assert np.array_equal(row_points.cpu().numpy()[:N], order) and row_points[N].item() == -7
    return pr, row_start, row_points


def _point_case(M, NC, N, dual, wide, seed):
    """Inputs of one forward + backward, their device copies, and the float64 reference of the forward."""
    rng = np.random.Generator(np.random.PCG64(seed))
    point_row, A = _point_rows(rng, N)
    ld, col = (M + 8, 4) if wide else (M, 0)
    ybuf = np.full((A, ld), np.nan, np.float32)          # the neighbouring channels of the slice: a NaN that leaks shows
    y = rng.standard_normal((A, M), dtype=np.float32)
    ybuf[:, col:col + M] = y
    w1, b1 = rng.standard_normal((NC, M), dtype=np.float32), rng.standard_normal(NC, dtype=np.float32)
    w2, b2 = (rng.standard_normal((NC, M), dtype=np.float32), rng.standard_normal(NC, dtype=np.float32)) if dual else (None, None)
    c = dict(M=M, NC=NC, N=N, A=A, ld=ld, col=col, dual=dual, point_row=point_row, y=y, w1=w1, b1=b1, w2=w2, b2=b2,
             dfeats=rng.standard_normal((N, M), dtype=np.float32), dl1=rng.standard_normal((N, NC), dtype=np.float32),
             dl2=rng.standard_normal((N, NC), dtype=np.float32) if dual else None,
             g0=[rng.standard_normal(s, dtype=np.float32) for s in ((NC, M), (NC,), (NC, M), (NC,))])
    c["d"] = {k: _dev(v) for k, v in (("ybuf", ybuf), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("dfeats", c["dfeats"]),
                                      ("dl1", c["dl1"]), ("dl2", c["dl2"])) if v is not None}
    return c


def _point_forward(c):
    lib, d = _lib(), c["d"]
    M, NC, N, dual = c["M"], c["NC"], c["N"], c["dual"]
    feats = torch.full((N + 1, M), SENT, device="cuda")
    l1 = torch.full((N + 1, NC), SENT, device="cuda")
    l2 = torch.full((N + 1, NC), SENT, device="cuda")
    pr = _dev(c["point_row"])
    lib.call("mopa_output_layer_heads_fwd", lib.ptr(d["ybuf"], c["col"]), c["ld"], lib.ptr(pr), N, M, NC, lib.ptr(d["w1"]), lib.ptr(d["b1"]),
             lib.ptr(d.get("w2")), lib.ptr(d.get("b2")), lib.ptr(feats), lib.ptr(l1), lib.ptr(l2) if dual else None, lib.stream())
    x = c["y"][c["point_row"]]
    assert np.array_equal(feats.cpu().numpy()[:N], x), "feats is a copy of the gathered rows"
    x64 = x.astype(np.float64)
    for got, w, b in ((l1, c["w1"], c["b1"]), (l2, c["w2"], c["b2"])):
        if w is None:
            assert torch.equal(_bits(got), _bits(torch.full_like(got, SENT))), "logit2 of a single head is not written"
            continue
        ref = x64 @ w.astype(np.float64).T + b.astype(np.float64)
        mag = np.abs(x64) @ np.abs(w.astype(np.float64)).T + np.abs(b.astype(np.float64))
        _within(got.cpu().numpy()[:N], ref, 2 * (M + 1) * U * mag, f"logits {c['M'], NC, N}")   # n = M + 1: M products and the bias
    for t in (feats, l1, l2):   # the guard row behind every output
        assert torch.equal(_bits(t[N:]), _bits(torch.full_like(t[N:], SENT)))
    return feats[:N].contiguous()


def _point_backward(c, feats, row_start, row_points, null, accumulate):
    """null: which of dfeats / dl1 / dl2 is passed as NULL (or None: all present)."""
    lib, d = _lib(), c["d"]
    M, NC, N, A, ld, col, dual = c["M"], c["NC"], c["N"], c["A"], c["ld"], c["col"], c["dual"]
    has = {k: (k != null and (k != "dl2" or dual)) for k in ("dfeats", "dl1", "dl2")}
    dy = torch.full((A + 1, ld), SENT, device="cuda")
    grads = [_dev(g) for g in c["g0"]]
    ws = torch.empty(max(lib.query("mopa_output_layer_heads_bwd_workspace_bytes", N, M, NC), 256), dtype=torch.uint8, device="cuda")
    lib.call("mopa_output_layer_heads_bwd", *(lib.ptr(d[k]) if has[k] else None for k in ("dfeats", "dl1", "dl2")), lib.ptr(feats),
             lib.ptr(d["w1"]), lib.ptr(d.get("w2")), lib.ptr(row_start), lib.ptr(row_points), A, N, M, NC, lib.ptr(dy, col), ld,
             lib.ptr(grads[0]), lib.ptr(grads[1]), lib.ptr(grads[2]) if dual else None, lib.ptr(grads[3]) if dual else None,
             accumulate, lib.ptr(ws), ws.numel(), lib.stream())
    # dy[row] = sum over the row's points of dfeats + dl1 @ W1 + dl2 @ W2
    per, mag = np.zeros((N, M)), np.zeros((N, M))
    if has["dfeats"]:
        per += c["dfeats"].astype(np.float64)
        mag += np.abs(c["dfeats"].astype(np.float64))
    for k, w in (("dl1", c["w1"]), ("dl2", c["w2"])):
        if has[k]:
            per += c[k].astype(np.float64) @ w.astype(np.float64)
            mag += np.abs(c[k].astype(np.float64)) @ np.abs(w.astype(np.float64))
    rows = torch.from_numpy(c["point_row"].astype(np.int64))
    ref = torch.zeros(A, M, dtype=torch.float64).index_add_(0, rows, torch.from_numpy(per)).numpy()
    smag = torch.zeros(A, M, dtype=torch.float64).index_add_(0, rows, torch.from_numpy(mag)).numpy()
    cnt = np.bincount(c["point_row"], minlength=A).astype(np.float64)
    got = dy.cpu().numpy()
    tag = f"{M, NC, N, null, accumulate}"
    _within(got[:A, col:col + M], ref, 2 * (cnt[:, None] * (2 * NC + 1)) * U * smag, "dy " + tag)   # n = points in the row * (2 NC + 1)
    empty = cnt == 0
    assert empty.any() and (_bits(dy[:A, col:col + M])[torch.from_numpy(empty)] == 0).all(), "rows without a point: +0.0 exactly"
    keep = np.ones((A + 1, ld), bool)
    keep[:A, col:col + M] = False   # everything outside the slice, and the guard row, keeps the pre-fill
    assert (_bits(dy)[torch.from_numpy(keep)] == _bits(torch.full((1,), SENT))[0]).all(), "dy wrote outside its channel slice"
    # dW[k][c] = sum_p dl[p][k] feats[p][c], db[k] = sum_p dl[p][k], added to the pre-fill when accumulate
    f64 = c["y"][c["point_row"]].astype(np.float64)
    for h, k in enumerate(("dl1", "dl2")):
        gw, gb = grads[2 * h].cpu().numpy(), grads[2 * h + 1].cpu().numpy()
        w0, b0 = c["g0"][2 * h], c["g0"][2 * h + 1]
        if not has[k]:
            assert np.array_equal(gw, w0) and np.array_equal(gb, b0), f"the head without a gradient keeps its buffers ({tag})"
            continue
        g = c[k].astype(np.float64)
        base_w, base_b = (w0.astype(np.float64), b0.astype(np.float64)) if accumulate else (0.0, 0.0)
        _within(gw, base_w + g.T @ f64, 2 * N * U * (np.abs(base_w) + np.abs(g).T @ np.abs(f64)), f"dW{h + 1} " + tag)   # n = N points
        _within(gb, base_b + g.sum(0), 2 * N * U * (np.abs(base_b) + np.abs(g).sum(0)), f"db{h + 1} " + tag)            # n = N points


@pytest.mark.parametrize("M,NC", POINT_CASES)
def test_point_heads_vs_fp64(M, NC):
    """Forward and backward of the point heads at (M, NC): N in {1, 63, 1024 + 4 PL + 3} (PL = points per block pass: two weight-
    gradient blocks, the four-in-flight loop, its remainder loop, a partial last lane group), single and dual head, a dense buffer
    and a channel slice, every gradient null in turn, accumulate 0 / 1 into pre-filled dW / db."""
    PL = 256 // _lanes(M)
    for i, (N, dual, wide) in enumerate(itertools.product((1, 63, 1024 + 4 * PL + 3), (False, True), (False, True))):
        assert N <= 2100
        c = _point_case(M, NC, N, dual, wide, seed=1000 * M + 10 * NC + i)
        _, row_start, row_points = _csr(c["point_row"], c["A"])
        feats = _point_forward(c)
        for null in (None, "dfeats", "dl1") + (("dl2",) if dual else ()):
            for accumulate in (0, 1):
                _point_backward(c, feats, row_start, row_points, null, accumulate)


def _raises_arg(name, *args):
    with pytest.raises(RuntimeError, match=rf"{name} failed with code -1$"):
        _lib().call(name, *args)


@pytest.mark.parametrize("M", POINT_M)
def test_point_heads_refuse_the_first_class_count_outside_the_limit(M):
    """Argument checks only: nothing is launched, and forward and backward refuse the same count."""
    lib = _lib()
    NC, N, A = point_limit(M) + 1, 5, 4
    assert not lib.query("mopa_heads_supported", M, NC) and lib.query("mopa_heads_supported", M, NC - 1)
    z = lambda *s: torch.zeros(*s, device="cuda")
    outs = [torch.full(s, SENT, device="cuda") for s in ((N, M), (N, NC), (N, NC), (A, M), (NC, M), (NC,), (NC, M), (NC,))]
    pr = torch.zeros(N, dtype=torch.int32, device="cuda")
    rs = torch.tensor([0, N, N, N, N], dtype=torch.int32, device="cuda")
    rp = torch.arange(N, dtype=torch.int32, device="cuda")
    y, w, b, g, gl = z(A, M), z(NC, M), z(NC), z(N, M), z(N, NC)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    p = lib.ptr
    _raises_arg("mopa_output_layer_heads_fwd", p(y), M, p(pr), N, M, NC, p(w), p(b), p(w), p(b), p(outs[0]), p(outs[1]), p(outs[2]),
                lib.stream())
    _raises_arg("mopa_output_layer_heads_bwd", p(g), p(gl), p(gl), p(g), p(w), p(w), p(rs), p(rp), A, N, M, NC, p(outs[3]), M,
                p(outs[4]), p(outs[5]), p(outs[6]), p(outs[7]), 0, p(ws), ws.numel(), lib.stream())
    torch.cuda.synchronize()
    for t in outs:
        assert torch.equal(_bits(t), _bits(torch.full_like(t, SENT)))


# ---------------------------------------------------------------------------------------------------------------- full-image head
PIXEL_SHAPES = ((1, 16, 16, 1, 1), (2, 16, 32, 13, 27), (2, 32, 32, 23, 27))   # 1, 702 and 1,242 pixels


def _pixel_run(M, NC, shape, wide, acc_dx, acc_params, seed):
    lib = _lib()
    B, Hp, Wp, H, W = shape
    rng = np.random.Generator(np.random.PCG64(seed))
    ld, col = (M + 8, 4) if wide else (M, 0)
    xbuf = np.full((B, Hp, Wp, ld), np.nan, np.float32)
    x = rng.standard_normal((B, Hp, Wp, M), dtype=np.float32)
    xbuf[..., col:col + M] = x
    w, b = rng.standard_normal((NC, M), dtype=np.float32), rng.standard_normal(NC, dtype=np.float32)
    dpred = rng.standard_normal((B, H, W, NC), dtype=np.float32)
    dx0 = rng.standard_normal((B, Hp, Wp, ld), dtype=np.float32)          # what accumulate_dx adds to; else the sentinel
    dw0, db0 = rng.standard_normal((NC, M), dtype=np.float32), rng.standard_normal(NC, dtype=np.float32)
    xd, wd, bd, dpd = _dev(xbuf), _dev(w), _dev(b), _dev(dpred)
    p = lib.ptr
    tag = f"{M, NC, shape, wide, acc_dx, acc_params}"

    pred = torch.full((B * H * W + 1, NC), SENT, device="cuda")
    lib.call("mopa_pixel_head_fwd", p(xd, col), ld, B, Hp, Wp, H, W, M, NC, p(wd), p(bd), p(pred), lib.stream())
    xin = x[:, :H, :W].astype(np.float64).reshape(-1, M)
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    _within(pred.cpu().numpy()[:-1], xin @ w64.T + b64, 2 * (M + 1) * U * (np.abs(xin) @ np.abs(w64).T + np.abs(b64)),
            "pred " + tag)                                                    # n = M + 1: M products and the bias
    assert torch.equal(_bits(pred[-1]), _bits(torch.full_like(pred[-1], SENT)))

    runs = []
    for _ in range(2):
        dx = _dev(dx0) if acc_dx else torch.full((B, Hp, Wp, ld), SENT, device="cuda")
        dw, db = _dev(dw0), _dev(db0)
        ws = torch.empty(max(lib.query("mopa_pixel_head_bwd_workspace_bytes", B, H, W, M, NC), 256), dtype=torch.uint8, device="cuda")
        lib.call("mopa_pixel_head_bwd", p(dpd), p(xd, col), ld, B, Hp, Wp, H, W, M, NC, p(wd), p(dx, col), ld, acc_dx, p(dw), p(db),
                 acc_params, p(ws), ws.numel(), lib.stream())
        runs.append((dx, dw, db))
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(_bits(a), _bits(c)), "ordered reductions: the same bits run to run (" + tag + ")"
    dx, dw, db = runs[0]
    g = dpred.astype(np.float64).reshape(-1, NC)
    base = dx0[:, :H, :W, col:col + M].astype(np.float64).reshape(-1, M) if acc_dx else 0.0
    got = dx.cpu().numpy()
    _within(got[:, :H, :W, col:col + M].reshape(-1, M), base + g @ w64, 2 * (NC + 1) * U * (np.abs(base) + np.abs(g) @ np.abs(w64)),
            "dx " + tag)                                                      # n = NC + 1: NC products and the value added to
    keep = np.ones((B, Hp, Wp, ld), bool)
    keep[:, :H, :W, col:col + M] = False   # outside the H x W window and outside the channel slice: bit for bit what was there
    before = _bits(_dev(dx0)) if acc_dx else _bits(torch.full((B, Hp, Wp, ld), SENT))
    assert torch.equal(_bits(dx)[torch.from_numpy(keep)], before[torch.from_numpy(keep)]), "dx outside the window changed (" + tag + ")"
    n = B * H * W
    bw, bb = (dw0.astype(np.float64), db0.astype(np.float64)) if acc_params else (0.0, 0.0)
    _within(dw.cpu().numpy(), bw + g.T @ xin, 2 * n * U * (np.abs(bw) + np.abs(g).T @ np.abs(xin)), "dW " + tag)   # n = B H W pixels
    _within(db.cpu().numpy(), bb + g.sum(0), 2 * n * U * (np.abs(bb) + np.abs(g).sum(0)), "db " + tag)             # n = B H W pixels


@pytest.mark.parametrize("M,NC", PIXEL_CASES)
def test_pixel_head_vs_fp64(M, NC):
    """Lanes per pixel 4, 16, 32, 64 (the DPP row sum alone, then one and two shuffle steps); 1, 702 and 1,242 pixels (less than one
    block pass, no multiple of the pixels per pass, two weight-gradient blocks); dense and sliced buffers; every accumulate flag."""
    for i, (shape, wide, acc_dx, acc_params) in enumerate(itertools.product(PIXEL_SHAPES, (False, True), (0, 1), (0, 1))):
        _pixel_run(M, NC, shape, wide, acc_dx, acc_params, seed=7000 * M + 100 * NC + i)


@pytest.mark.parametrize("M", PIXEL_M)
def test_pixel_head_refuses_the_first_class_count_outside_the_limit(M):
    """Argument checks only, before the first launch: dx, dW and db of a refused backward keep their bits."""
    lib = _lib()
    NC = pixel_limit(M) + 1
    assert not lib.query("mopa_pixel_head_supported", M, NC) and lib.query("mopa_pixel_head_supported", M, NC - 1)
    B, Hp, Wp, H, W = 1, 16, 16, 3, 5
    z = lambda *s: torch.zeros(*s, device="cuda")
    outs = [torch.full(s, SENT, device="cuda") for s in ((B * H * W, NC), (B * Hp * Wp, M), (NC, M), (NC,))]
    x, w, b, dp = z(B * Hp * Wp, M), z(NC, M), z(NC), z(B * H * W, NC)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    p = lib.ptr
    _raises_arg("mopa_pixel_head_fwd", p(x), M, B, Hp, Wp, H, W, M, NC, p(w), p(b), p(outs[0]), lib.stream())
    _raises_arg("mopa_pixel_head_bwd", p(dp), p(x), M, B, Hp, Wp, H, W, M, NC, p(w), p(outs[1]), M, 0, p(outs[2]), p(outs[3]), 0, p(ws),
                ws.numel(), lib.stream())
    torch.cuda.synchronize()
    for t in outs:
        assert torch.equal(_bits(t), _bits(torch.full_like(t, SENT)))


# ---------------------------------------------------------------------------------------------------------------- the networks
def test_networks_refuse_16_classes_when_built_and_train_with_15():
    """The class limit surfaces where the model is built (16 classes: no 64- or 16-wide head), and the largest supported count runs a
    whole step -- forward, losses, backward -- on a 32 x 48 image and about 500 voxels, its logits the heads' own features times
    the weights in float64."""
    from mopa_amd import synth
    from mopa_amd.common.utils.loss import seg_ce, xm_kl
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d, build_model_3d
    with pytest.raises(ValueError, match=r"Net2DSeg: 16 classes at feature width 64.*1\.\.15 classes"):
        build_model_2d(default_cfg(num_classes=16))
    with pytest.raises(ValueError, match=r"Net3DSeg: 16 classes at feature width 16.*1\.\.15 classes"):
        build_model_3d(default_cfg(num_classes=16))
    NC = 15
    assert NC == point_limit(64) == point_limit(16) == pixel_limit(64)
    torch.manual_seed(0)
    cfg = default_cfg(num_classes=NC)
    cfg.MODEL_3D.SCN.num_planes = 4
    m3, m2 = build_model_3d(cfg)[0].cuda().train(), build_model_2d(cfg)[0].cuda().train()
    pts = synth.lidar_points(0)
    pts = pts[::max(1, len(pts) // 500)]
    n = len(pts)
    coords = np.concatenate([synth.voxelize(pts), np.zeros((n, 1), np.int64)], 1)
    rng = np.random.Generator(np.random.PCG64(0))
    H, W = 32, 48
    batch = {"x": [torch.from_numpy(coords), torch.ones(n, 1)], "img": torch.from_numpy(rng.random((1, 3, H, W), dtype=np.float32)),
             "img_indices": [np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], 1)]}
    label = torch.from_numpy(rng.integers(0, NC, n)).cuda()
    o3, o2 = m3(batch), m2(batch)
    assert o2["seg_logit_all"].shape == (1, H, W, NC) and o3["seg_logit"].shape == (n, NC)
    for o, m in ((o2, m2), (o3, m3)):
        f = o["feats"].detach().cpu().double()
        for key, lin in (("seg_logit", m.linear), ("seg_logit2", m.linear2)):
            ref = f @ lin.weight.detach().cpu().double().T + lin.bias.detach().cpu().double()
            mag = f.abs() @ lin.weight.detach().cpu().double().abs().T + lin.bias.detach().cpu().double().abs()
            _within(o[key].detach().cpu().numpy(), ref.numpy(), 2 * (f.shape[1] + 1) * U * mag.numpy(), key)   # n = M + 1
    l2 = seg_ce(o2["seg_logit"], label) + xm_kl(o2["seg_logit2"], o3["seg_logit"]) + o2["seg_logit_all"].square().mean()
    l3 = seg_ce(o3["seg_logit"], label) + xm_kl(o3["seg_logit2"], o2["seg_logit"])
    l2.backward()
    l3.backward()
    torch.cuda.synchronize()
    for m in (m2, m3):
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
        assert m.linear.weight.grad.abs().sum() > 0 and m.linear2.weight.grad.abs().sum() > 0
