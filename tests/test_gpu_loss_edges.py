"""Edges of the loss, optimiser and column-sum kernels against float64: class counts 1 .. 64 and row counts on both sides of a
block and past the grid (csrc/losses.hip's stride loops), logit ranges where exp(z - lse) underflows, label edge cases of the
weighted CE, the three wave-count branches of k_mc_pass (mask consistency), k_adam_flat's scalar tail and k_colsum_partial at widths
with idle threads.  References: oracle/losses.py in float64, Adam written out from the formula in csrc/optim.hip's header, a float64
column sum.  tests/test_gpu_losses.py keeps the golden vectors and the full-size cases."""
import math

import numpy as np
import pytest
import torch

from oracle import losses as olosses

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _lib():
    from mopa_amd import _lib
    return _lib


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _t64(x):
    return (torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else torch.as_tensor(x)).detach().cpu().double()


def _within(got, ref, bound, what, rtol=0.0):
    """|got - ref| <= bound + rtol |ref| elementwise in float64; a NaN anywhere fails."""
    got, ref = _t64(got), _t64(ref)
    bound = _t64(bound).expand_as(ref)
    if rtol:
        bound = ref.abs().mul_(rtol).add_(bound)
    err = (got - ref).abs_()
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(int(k) for k in np.unravel_index(int(torch.where(bad, err.nan_to_num(nan=float("inf")), -torch.ones(())).argmax()),
                                                   tuple(err.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} outside the bound; worst at {i}: got {got[i].item()!r}, "
                             f"want {ref[i].item()!r}, |err| {err[i].item():.3e} > {bound[i].item():.3e}")


# ------------------------------------------------------------------------------------------------ KL, CE, softmax
# The absolute error of a softmax gradient.  Every gradient entry is s * (p_c - t_c) with p_c = exp(z_c - lse) and t_c another
# softmax (KL) or 0 / 1 (CE).  lse = max + log(sum) is at most Z + log C in magnitude (Z = the row's largest |logit|) and is rounded
# once at that magnitude: |d lse| <= 2^-24 (Z + log C) plus a few ulp of log's and the sum's own (values <= log 64 = 4.2).  The
# argument a = z_c - lse is rounded at |a|, so |d a| <= 2^-24 (Z + |a| + c0) and p_c = e^a carries it amplified by p_c itself:
# |d p| <= p |d a| + ulp(p) <= 2^-24 ((Z + c0) e^a + |a| e^a + 1) <= 2^-24 (Z + c0 + 1.4) since |a| e^a <= 1/e.  With c0 ~ 2.6
# for expf, logf and the sum: |d p| <= (Z + 4) 2^-24, and two such terms (p and q of the KL; p and the scale's own rounding for CE)
# give (4 + 2 Z) 2^-23 s with room to spare.  s is the op's gradient scale: gout / N (KL), gout w[y] / den (CE).
def softmax_grad_bound(Z, s):
    return (4.0 + 2.0 * Z) * 2.0 ** -23 * s


def _loss_case(N, C, seed, wide=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    gen = torch.Generator().manual_seed(seed)
    a, b = torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen)
    dp = b.flip(1)   # the upstream gradient of the softmax: standard normal as well, and not another 33 M draws at the largest size
    if wide:   # rows scaled by 0, +-30, +-90: exp(z - lse) underflows to 0 in some classes of p and of q
        sa = torch.tensor([0., 30, -30, 90, -90])[torch.arange(N) % 5]
        sb = torch.tensor([90., 0, -90, 30, -30, 0, 30])[torch.arange(N) % 7]
        a, b = a * sa[:, None], b * sb[:, None]
    else:
        a, b = a * 4, b * 4
    lab = rng.integers(0, C, N)
    lab[rng.random(N) < 0.3] = -100
    if N == 1:
        lab[:] = C - 1
    w = rng.uniform(1, 3, C).astype(np.float32)
    return a, b, torch.from_numpy(lab), torch.from_numpy(w), dp


def _chunked(N, size=65536):
    return [(i, min(i + size, N)) for i in range(0, N, size)]


def _check_kl_ce_softmax(N, C, seed, wide):
    """Values against oracle/losses.py over ALL rows (in pieces of 65,536 rows: the oracle's means recombined with their row counts
    / weight sums); gradients and probabilities against it on every row up to 4,096 rows and, above that, on every 61st row and
    the last five (the rows of the stride loop): a row's gradient depends on its own logits and on the global normaliser only,
    so the oracle on the subset, rescaled by (subset normaliser / global normaliser), is the reference of those rows.  The device
    results of all rows are checked to be finite."""
    from mopa_amd.common.utils.loss import seg_ce, softmax_lastdim, xm_kl
    a, b, lab, w, dp = _loss_case(N, C, seed, wide)
    idx = torch.arange(N) if N <= 4096 else torch.unique(torch.cat([torch.arange(0, N, 61), torch.arange(N - 5, N)]))
    w64 = w.double()
    keep = lab >= 0
    den = w64[lab[keep]].sum().item()
    klr = cer = 0.0
    with torch.no_grad():
        for i, j in _chunked(N):
            klr += olosses.xm_kl(a[i:j].double(), b[i:j].double()).item() * (j - i) / N
            if keep[i:j].any():
                cer += olosses.seg_ce(a[i:j].double(), lab[i:j], w64).item() * w64[lab[i:j][keep[i:j]]].sum().item() / den
    a_s, b_s, lab_s = a[idx], b[idx], lab[idx]
    ar = a_s.double().requires_grad_(True)
    ad = a.cuda().requires_grad_(True)
    gk, gc = 1.75, 0.625   # upstream gradients of the two losses (exact in fp32)
    kl = xm_kl(ad, b.cuda())
    assert math.isfinite(kl.item())
    np.testing.assert_allclose(kl.item(), klr, rtol=1e-5, atol=1e-12 if C == 1 else 0)   # (C = 1: the value is 0)
    Za = a_s.abs().amax(1).double().numpy()
    Zab = np.maximum(Za, b_s.abs().amax(1).double().numpy())
    (gka,) = torch.autograd.grad(kl * gk, ad)
    (gkr,) = torch.autograd.grad(olosses.xm_kl(ar, b_s.double()) * (gk * len(idx) / N), ar)
    assert torch.isfinite(gka).all()
    gka = gka.cpu()
    # ordinary inputs: the tolerances of tests/test_gpu_losses.py (rtol 1e-4) over the derived absolute bound; wide rows: the bound
    _within(gka[idx], gkr, softmax_grad_bound(Zab, gk / N)[:, None], f"d KL {N, C, wide}", rtol=0 if wide else 1e-4)
    if wide:
        # a class whose q underflowed adds exactly 0 to the value (the `q > 0 ? ... : 0` branch) and has the gradient g * (p - 0);
        # one whose p underflowed has g * (0 - q): the same expf(z - lse) as the softmax kernel and g = gout / N in fp32, so the
        # bits of g * p and -g * q are known
        g32 = torch.tensor(gk, dtype=torch.float32) / torch.tensor(float(N), dtype=torch.float32)
        pd, qd = softmax_lastdim(a.cuda()).cpu(), softmax_lastdim(b.cuda()).cpu()
        q0, p0 = torch.softmax(b.double(), 1) < 1e-60, torch.softmax(a.double(), 1) < 1e-60
        assert q0.any() and p0.any() and (qd[q0] == 0).all() and (pd[p0] == 0).all()
        assert torch.equal(gka[q0], (g32 * (pd - qd))[q0]) and torch.equal(gka[q0 & ~p0], (g32 * pd)[q0 & ~p0])
        assert torch.equal(gka[p0 & ~q0], (-g32 * qd)[p0 & ~q0])
        assert (gka[p0 & q0] == 0).all()

    ce = seg_ce(ad, lab.cuda(), w.cuda())
    assert math.isfinite(ce.item())
    np.testing.assert_allclose(ce.item(), cer, rtol=1e-5, atol=1e-12 if C == 1 else 0)
    (gca,) = torch.autograd.grad(ce * gc, ad)
    keep_s = lab_s >= 0
    den_s = w64[lab_s[keep_s]].sum().item()
    (gcr,) = torch.autograd.grad(olosses.seg_ce(ar, lab_s, w64) * (gc * den_s / den), ar)
    s = torch.where(keep_s, w64[lab_s.clamp(min=0)], torch.zeros((), dtype=torch.float64)).numpy() * gc / den
    assert torch.isfinite(gca).all()
    gca = gca.cpu()
    _within(gca[idx], gcr, softmax_grad_bound(Za, s)[:, None], f"d CE {N, C, wide}", rtol=0 if wide else 1e-4)
    assert (gca[~keep] == 0).all()

    zd = a.cuda().requires_grad_(True)
    p = softmax_lastdim(zd)
    pr = torch.softmax(ar, 1)
    # one p, s = 1: half the two-term bound
    _within(p.detach().cpu()[idx], pr, softmax_grad_bound(Za, 1.0)[:, None] / 2, f"softmax {N, C, wide}", rtol=0 if wide else 1e-5)
    (gz,) = torch.autograd.grad(p, zd, dp.cuda())
    (gzr,) = torch.autograd.grad(pr, ar, dp[idx].double())
    assert torch.isfinite(p).all() and torch.isfinite(gz).all()
    # dz = p (dp - sum_c dp p): the error of p against |dp - dot| <= 2 D (D = the row's largest |dp|), the dot's own C + 1 roundings
    # and the C errors of p inside it (their sum is bounded like one p, the p summing to 1): s = 2 D, plus 2 (C + 1) 2^-24 D
    D = dp[idx].abs().amax(1).double().numpy()
    _within(gz.cpu()[idx], gzr, (softmax_grad_bound(Za, 2 * D) + 2 * (C + 1) * U * D)[:, None], f"d softmax {N, C, wide}",
            rtol=0 if wide else 1e-4)


@pytest.mark.parametrize("N", (1, 255, 257, 2048 * 256 + 5))
@pytest.mark.parametrize("C", (1, 2, 11, 64))
def test_kl_ce_softmax_value_and_gradient(N, C):
    """N below / above one block of 256 rows and five rows past the grid's 2048 x 256 threads (the stride loops)."""
    _check_kl_ce_softmax(N, C, seed=100 * C + N % 97, wide=False)


@pytest.mark.parametrize("C", (11, 64))
def test_kl_ce_softmax_wide_logit_range(C):
    _check_kl_ce_softmax(1030, C, seed=5 + C, wide=True)


def test_seg_ce_label_edges():
    from mopa_amd.common.utils.loss import seg_ce
    lib = _lib()
    rng = np.random.Generator(np.random.PCG64(21))
    N, C = 700, 11
    z = torch.from_numpy(rng.standard_normal((N, C), dtype=np.float32) * 4)
    lab = torch.from_numpy(rng.integers(0, C, N))
    lab[rng.random(N) < 0.2] = -100
    w = torch.from_numpy(rng.uniform(1, 3, C).astype(np.float32))
    w[4] = 0.0                                                       # a class whose weight is 0
    assert (lab == 4).any()
    zr = z.double().requires_grad_(True)
    ref = olosses.seg_ce(zr, lab, w.double())
    ref.backward()
    Z = z.abs().amax(1).double().numpy()
    keep = lab >= 0
    den = w.double()[lab[keep]].sum().item()
    s = torch.where(keep, w.double()[lab.clamp(min=0)], torch.zeros((), dtype=torch.float64)).numpy() / den
    for dtype in (torch.int32, torch.int64):                         # labels as int32 and int64: the same bits
        zd = z.cuda().requires_grad_(True)
        ce = seg_ce(zd, lab.to(dtype).cuda(), w.cuda())
        np.testing.assert_allclose(ce.item(), ref.item(), rtol=1e-5)
        ce.backward()
        _within(zd.grad, zr.grad, softmax_grad_bound(Z, s)[:, None], f"d CE {dtype}", rtol=1e-4)
        assert (zd.grad.cpu()[lab == 4] == 0).all() and (zd.grad.cpu()[lab == -100] == 0).all()
    # every row that is not ignored has weight 0: 0 / 0, NaN as torch gives it
    only4 = torch.where(lab == 4, lab, torch.full_like(lab, -100))
    assert torch.isnan(olosses.seg_ce(z.double(), only4, w.double()))
    assert torch.isnan(seg_ce(z.cuda(), only4.cuda(), w.cuda()))
    # labels outside [0, C) that are not the ignore index (here 7 is it, so -100 is outside as well): dropped from numerator and
    # normaliser, their gradient rows zero, the status word set
    bad = lab.clone()
    bad[0], bad[100], bad[256], bad[699] = C, 255, -1, 255
    ign = 7
    outside = (bad < 0) | (bad >= C)
    assert outside.sum() > 4 and (bad == ign).any()
    clean = torch.where(outside | (bad == ign), torch.full_like(bad, -100), bad)
    zr2 = z.double().requires_grad_(True)
    ref2 = olosses.seg_ce(zr2, clean, w.double())
    ref2.backward()
    zd = z.cuda().requires_grad_(True)
    ce = seg_ce(zd, bad.cuda(), w.cuda(), ignore_index=ign)
    np.testing.assert_allclose(ce.item(), ref2.item(), rtol=1e-5)
    ce.backward()
    keep2 = clean >= 0
    s2 = torch.where(keep2, w.double()[clean.clamp(min=0)], torch.zeros((), dtype=torch.float64)).numpy() / w.double()[clean[keep2]].sum().item()
    _within(zd.grad, zr2.grad, softmax_grad_bound(Z, s2)[:, None], "d CE, bad labels", rtol=1e-4)
    assert (zd.grad.cpu()[~keep2] == 0).all()
    out, status = torch.zeros(2, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(lib.query("mopa_loss_workspace_bytes", N), 256), dtype=torch.uint8, device="cuda")
    zc, wc = z.cuda(), w.cuda()
    for labels, want in ((bad, 1), (clean, 0)):
        status.zero_()
        lc = labels.cuda()
        lib.call("mopa_wce_fwd", lib.ptr(zc), lib.ptr(lc), lib.ptr(wc), N, C, ign if want else -100, lib.ptr(out), lib.ptr(out, 1),
                 lib.ptr(status), lib.ptr(ws), ws.numel(), lib.stream())
        assert status.item() == want
        np.testing.assert_allclose(out[0].item(), ref2.item(), rtol=1e-5)


# ------------------------------------------------------------------------------------------------ mask consistency
MC_SHAPES = {1: (1, 1), 63: (7, 9), 65: (5, 13), 4095: (63, 65), 4097: (17, 241)}


def _mc_case(C, HW, seed):
    """probs (B, H, W, C) fp32 and B masks (H, W): ids 0 and 255, ids >= 256 and negative ids (ignored), a single-pixel mask, an image
    without a valid id, and a mask whose probability of class 0 is 0 on every pixel (mu = 0 under log2(mu + 1e-30))."""
    H, W = MC_SHAPES[HW]
    rng = np.random.Generator(np.random.PCG64(seed))
    B = 4
    probs = torch.softmax(torch.from_numpy(rng.standard_normal((B, H, W, C), dtype=np.float32)), 3)
    pool = np.asarray([0, 255, 17, 300, -1, 256, -100, 3])
    masks = np.empty((B, HW), np.int64)
    for b in range(B):
        run = np.repeat(pool[rng.integers(0, len(pool), HW // 5 + 2)], rng.integers(1, 11, HW // 5 + 2))   # runs of 1..10 pixels
        masks[b] = np.resize(run, HW)
    if HW == 1:
        masks[:, 0] = [0, 255, 300, 17]          # one pixel per image: every mask is a single-pixel mask
    else:
        masks[0, :2] = [0, 255]
        masks[0, HW // 2] = 99                    # the single-pixel mask
        masks[0, -1] = 3                          # a valid id on the last pixel: the tail of the last 64-pixel group counts
        masks[1, 0], masks[1, -1] = 256, -1
        masks[3, :3] = [17, 300, 17]
    masks[2] = np.where(np.arange(HW) % 2 == 0, 300, -1)   # no valid id: adds 0, counts in the mean, zero gradient
    masks = masks.reshape(B, H, W)
    probs[torch.from_numpy(masks == 17)] *= torch.cat([torch.zeros(1), torch.ones(C - 1)])   # class 0 is 0 all over mask 17
    for wanted in (0, 255, 17, 300) + ((-1, 256, 99) if HW > 1 else ()):
        assert (masks == wanted).any()
    return probs, masks.astype(np.int32)


@pytest.mark.parametrize("min_entropy", (False, True))
@pytest.mark.parametrize("HW", sorted(MC_SHAPES))
@pytest.mark.parametrize("C", (1, 15, 16, 31, 32))
def test_mask_cons_wave_branches_vs_oracle(C, HW, min_entropy):
    """k_mc_pass runs 4 waves per block up to C = 15, 2 up to 31 and 1 at 32 (its accumulators in 64 KiB of LDS); the count lane is
    lane C.  Value and gradient against oracle/losses.py in float64, the masks' ids >= 256 set to -1 for the oracle (the documented
    deviation); two runs give the same bits."""
    from mopa_amd.common.utils.loss import mask_cons_loss
    probs, masks = _mc_case(C, HW, seed=10 * C + HW)
    B, H, W, _ = probs.shape
    mlist = [torch.from_numpy(m) for m in masks]
    if H == 1 and min_entropy:
        # the entropy term is normalised by log2(H) = 0 for a one-row image (the reference divides by it): refused, nothing launched
        with pytest.raises(RuntimeError, match=r"mopa_mask_cons_fwd failed with code -1$"):
            mask_cons_loss(probs.cuda(), mlist, True)
        return
    runs = []
    for _ in range(2):
        pd = probs.cuda().requires_grad_(True)
        loss = mask_cons_loss(pd, mlist, min_entropy)
        (loss * 1.5).backward()
        runs.append((loss.detach(), pd.grad))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    pr = probs.double().requires_grad_(True)
    omasks = [torch.from_numpy(np.where(m >= 256, -1, m)) for m in masks]
    ref = olosses.mask_cons_loss(pr, omasks, min_entropy)
    (ref * 1.5).backward()
    loss, grad = runs[0]
    assert math.isfinite(loss.item())
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-5, atol=1e-12 if C == 1 else 0)   # (C = 1: the value is 0)
    # gradient: rtol 1e-3 as tests/test_gpu_losses.py, and an absolute part for entries that cancel, scaled to 1 / (B n C): an entry is
    # g / (B M_b) [2 (P - mu) / (n C) - (log2(mu + 1e-30) + 1 / ln 2) / (n log2 H)].  mu is an ordered fp32 sum -- a 6-step butterfly,
    # at most 64 group sums of one wave in a block, 3 wave sums, the blocks in double -- so it carries at most 73 roundings of at
    # most the whole sum, |d mu| <= 80 * 2^-24 mu <= 80 * 2^-24; that is the error of P - mu, and 1 / ln 2 times it that of log2(mu)
    n = np.ones((B, H * W))
    flat = np.where(masks.reshape(B, -1) >= 256, -1, masks.reshape(B, -1))
    for b in range(B):
        ids, inv, cnt = np.unique(flat[b], return_inverse=True, return_counts=True)
        n[b] = cnt[inv]
    atol = 1.5 / B * 80 * U * (2.0 / (n * C) + (1.5 / (n * math.log2(H)) if min_entropy else 0.0))
    _within(grad.reshape(B, H * W, C), pr.grad.reshape(B, H * W, C), atol[:, :, None], f"d mask_cons {C, HW, min_entropy}", rtol=1e-3)
    assert (grad.cpu().numpy().reshape(B, H * W, C)[flat < 0] == 0).all()          # ignored pixels, the image without a valid id


def test_mask_cons_refuses_33_classes():
    from mopa_amd.common.utils.loss import mask_cons_loss
    probs = torch.full((1, 4, 4, 33), 1 / 33, device="cuda")
    with pytest.raises(RuntimeError, match=r"mopa_mask_cons_fwd failed with code -1$"):
        mask_cons_loss(probs, [torch.zeros(4, 4, dtype=torch.int32)], False)


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("grad_scale", (1.0, 0.5))
@pytest.mark.parametrize("weight_decay", (0.0, 0.01))
@pytest.mark.parametrize("n", (1, 2, 3, 5, 4 * 300 + 3))
def test_adam_flat_scalar_tail_vs_fp64(n, weight_decay, grad_scale):
    """mopa_adam_flat at lengths that are no multiple of 4 (FlatAdam pads every parameter, so its scalar tail never runs there):
    five steps, each compared with the formula of csrc/optim.hip's header in float64 FROM THE DEVICE'S OWN fp32 STATE, so that one
    step's roundings are what is measured: a few ulp of p, m and v, rtol 1e-6.  |p| and |g| stay above 0.1 and a gradient keeps its
    sign over the steps, so that neither b1 m + (1 - b1) g nor p - update cancels and a relative bound means something."""
    lib = _lib()
    rng = np.random.Generator(np.random.PCG64(n * 7 + int(weight_decay * 100) + int(grad_scale * 10)))
    stride = (n + 4 + 3) // 4 * 4                      # every buffer 16-byte aligned inside ONE allocation, >= 4 guard floats behind n
    GUARD = 7.0e7
    buf = torch.full((4 * stride,), GUARD, device="cuda")
    assert buf.data_ptr() % 16 == 0
    views = [buf[i * stride:i * stride + n] for i in range(4)]   # p, g, m, v
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    views[0].copy_(torch.from_numpy((sign * (0.1 + np.abs(rng.standard_normal(n)))).astype(np.float32)))   # (g + wd p: one sign)
    views[2].zero_()
    views[3].zero_()
    f32 = lambda x: float(np.float32(x))               # the scalars as the kernel receives them
    lr, b1, b2, eps, wd, gs = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(weight_decay), f32(grad_scale)
    for t in range(1, 6):
        views[1].copy_(torch.from_numpy((sign * (0.1 + np.abs(rng.standard_normal(n)))).astype(np.float32)))
        p0, g, m0, v0 = (v.cpu().double().numpy() for v in views)
        bc1, bc2s = f32(1 - 0.9 ** t), f32(math.sqrt(1 - 0.999 ** t))
        lib.call("mopa_adam_flat", lib.ptr(views[0]), lib.ptr(views[1]), lib.ptr(views[2]), lib.ptr(views[3]), n, lr, b1, b2, eps, wd,
                 bc1, bc2s, gs, lib.stream())
        gg = g * gs + wd * p0
        m = b1 * m0 + (1 - b1) * gg
        v = b2 * v0 + (1 - b2) * gg * gg
        p = p0 - lr / bc1 * m / (np.sqrt(v) / bc2s + eps)
        for name, got, want in (("p", views[0], p), ("m", views[2], m), ("v", views[3], v)):
            np.testing.assert_allclose(got.cpu().double().numpy(), want, rtol=1e-6, atol=0, err_msg=f"{name} after step {t}")
        assert np.array_equal(views[1].cpu().double().numpy(), g)
    guards = torch.ones(4 * stride, dtype=torch.bool)
    for i in range(4):
        guards[i * stride:i * stride + n] = False
    assert torch.equal(_bits(buf)[guards], _bits(torch.full((int(guards.sum()),), GUARD))), "a float behind n was written"


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("rows", (1, 31, 33, 4099))
@pytest.mark.parametrize("C", (4, 12, 64, 516, 1024))
def test_colsum_vs_fp64(C, rows):
    """C / 4 = 1, 3, 16, 129, 256 float4 columns: 256, 85, 16, 1 and 1 row lanes per block, with 0, 1, 0, 127 and 0 idle threads;
    rows around one block's 32 and in 129 blocks.  A channel slice of a wider buffer (NaN beside it), accumulate 0 / 1."""
    lib = _lib()
    rng = np.random.Generator(np.random.PCG64(C * 31 + rows))
    ld, col = C + 8, 4
    x = rng.standard_normal((rows, C), dtype=np.float32)
    xbuf = np.full((rows, ld), np.nan, np.float32)
    xbuf[:, col:col + C] = x
    xd = torch.from_numpy(xbuf).cuda()
    out0 = rng.standard_normal(C, dtype=np.float32)
    ws = torch.empty(max(lib.query("mopa_colsum_workspace_bytes", rows, C), 256), dtype=torch.uint8, device="cuda")
    x64 = x.astype(np.float64)
    for accumulate in (0, 1):
        out = torch.full((C + 4,), -3.25, device="cuda")
        out[:C] = torch.from_numpy(out0).cuda()
        lib.call("mopa_colsum", lib.ptr(xd, col), ld, rows, C, lib.ptr(out), accumulate, lib.ptr(ws), ws.numel(), lib.stream())
        base = out0.astype(np.float64) if accumulate else np.zeros(C)
        # n = rows terms (and the value added to): 2 n 2^-24 sum|terms|
        _within(out.cpu().numpy()[:C], base + x64.sum(0), 2 * rows * U * (np.abs(base) + np.abs(x64).sum(0)), f"colsum {C, rows, accumulate}")
        assert (out[C:] == -3.25).all()
    assert torch.equal(_bits(xd), _bits(torch.from_numpy(xbuf)))


@pytest.mark.parametrize("C", (1028, 6))
def test_colsum_refuses(C):
    lib = _lib()
    x = torch.zeros(8, 1032, device="cuda")
    out = torch.full((1032,), -3.25, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=r"mopa_colsum failed with code -1$"):
        lib.call("mopa_colsum", lib.ptr(x), 1032, 8, C, lib.ptr(out), 0, lib.ptr(ws), ws.numel(), lib.stream())
    torch.cuda.synchronize()
    assert (out == -3.25).all()
