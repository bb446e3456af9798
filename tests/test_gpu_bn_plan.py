"""What BnOp launches is what dense2d.bn_plan says, and it computes the BatchNorm: forward + backward against the fp64 formula under the
bounds of tests/test_gpu_bn_bwd_fused.py, on 2 G images of 6 x 10 (120 G rows: ragged against the 32-row blocks and against RL for every
C).  The stem forms ("sums", "sums_pool" and the weight gradients behind them) are the business of tests/test_gpu_stem_bwd.py's network
tests, the synchronised form of tests/test_gpu_syncbn.py."""
import numpy as np
import pytest
import torch

from test_gpu_bn_bwd_fused import TOL, TOL_DRES, _close
from test_gpu_conv_plan import _Recorder

EPS = 1e-5
FWD = {"stats": "mopa_bn_act_fwd_groups", "groups_bits": "mopa_bn_act_fwd_groups_bits", "groups": "mopa_bn_act_fwd_groups", "single": "mopa_bn_act_fwd"}
BWD = {"fused": "mopa_bn_act_bwd_groups_fused", "groups": "mopa_bn_act_bwd_groups", "single": "mopa_bn_act_bwd"}
# C, G, residual, biased producer, deferred, BN_MASK_BITS
CASES = [(C, G, res, biased, deferred, bits) for C in (48, 64, 256) for G in (1, 2)
         for res, biased, deferred, bits in ((False, False, False, True),    # plain
                                             (True, False, False, True),     # residual: bits where C % 32 == 0
                                             (True, False, False, False),    # residual, the saved output as the mask
                                             (False, True, False, True),     # behind a convolution with a bias
                                             (False, False, True, True),     # deferred
                                             (False, True, True, True))]     # deferred, behind a convolution with a bias


def _plans(d, C, G, res, biased, deferred):
    fwd = d.bn_plan(C, G, True, True, 1, res, deferred, False, biased)
    return fwd, d.bn_plan(C, G, True, True, 1, res, deferred, False, biased, bits=fwd.bits)


@pytest.mark.gpu
@pytest.mark.parametrize("C,G,res,biased,deferred,bits", CASES)
def test_bnop_runs_what_the_plan_says(C, G, res, biased, deferred, bits, monkeypatch):
    from mopa_amd import dense2d as d
    monkeypatch.setattr(d, "BN_MASK_BITS", bits)
    B, H, W = 2 * G, 6, 10
    rows, n = B * H * W, H * W * 2
    rng = np.random.Generator(np.random.PCG64([C, G, res, biased, deferred]))
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda()   # noqa: E731
    x, dy = d.Img(rnd(rows, C) * 2 + 1, B, H, W), d.Img(rnd(rows, C), B, H, W)
    r = d.Img(rnd(rows, C), B, H, W) if res else None
    P = {"bn.weight": rnd(C).abs() + 0.5, "bn.bias": rnd(C), "bn.running_mean": torch.zeros(C, device="cuda"),
         "bn.running_var": torch.ones(C, device="cuda")}
    fplan, bplan = _plans(d, C, G, res, biased, deferred)
    rec = _Recorder(monkeypatch, d)
    op = d.BnOp(P, "bn", 1, r, G, biased=biased)
    y = op.forward(x, None, True, True, deferred)
    assert rec.take() == [FWD[fplan.fwd]] * (G if fplan.fwd == "single" else 1)
    assert (op.bits is not None) == fplan.bits and hasattr(y, "bn") == deferred
    dres = d.new_img(B, H, W, C, "cuda") if res else None
    dg, db = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
    dx = op.backward(dy, dres, False, True, dg, db, False, False)
    assert op.plan(True) == bplan   # (after the forward pass: from what it left)
    assert rec.take() == [BWD[bplan.bwd]] * (G if bplan.bwd == "single" else 1)
    # fp64, per group; the activation mask is the stored output's sign or, deferred, that of x * scale + shift from the fp32 scale and
    # shift (the consumer's fused multiply-add rounds the exact value, so its sign is the exact value's)
    xd, gm, bt = x.t.double(), P["bn.weight"].double(), P["bn.bias"].double()
    st = op.stats.double().repeat_interleave(n, 0)
    dz = dy.t.double() * ((xd * st[:, 0] + st[:, 1]) > 0 if deferred else y.t > 0)
    yr, dxr, dgr, dbr = torch.empty_like(xd), torch.empty_like(xd), torch.zeros(C, dtype=torch.float64, device="cuda"), torch.zeros(C, dtype=torch.float64, device="cuda")
    for g in range(G):
        xs, zs = xd[g * n:(g + 1) * n], dz[g * n:(g + 1) * n]
        inv = 1.0 / torch.sqrt(xs.var(0, unbiased=False) + EPS)
        xhat = (xs - xs.mean(0)) * inv
        yr[g * n:(g + 1) * n] = torch.relu(xhat * gm + bt + (r.t.double()[g * n:(g + 1) * n] if res else 0.0))
        dbr += zs.sum(0)
        dgr += (zs * xhat).sum(0)
        dxr[g * n:(g + 1) * n] = gm * inv * (zs - zs.mean(0) - xhat * (zs * xhat).mean(0))
    if not deferred:
        _close(y.t, yr, *TOL)
    _close(dx.t, dxr, *TOL)
    _close(dg, dgr, *TOL)
    _close(db, dbr, *TOL)
    if res:
        _close(dres.t, dz, *TOL_DRES)
    # the partial column sums travel with the gradient: their reduction is mopa_colsum of the dx that was written, bit for bit
    assert (getattr(dx, "partial", None) is not None) == bplan.colsum
    if bplan.colsum:
        a, b = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        d.colsum(dx, a)
        d.colsum(dx, b, partial=dx.partial)
        assert torch.equal(a, b)


def test_every_form_is_reached_by_the_cases_above(monkeypatch):
    """(A size computation: every form but the synchronised one and the stem's is reached, in each pass.)"""
    from mopa_amd import dense2d as d
    seen = {"fwd": set(), "bwd": set(), "bits": set(), "colsum": set()}
    for C, G, res, biased, deferred, bits in CASES:
        monkeypatch.setattr(d, "BN_MASK_BITS", bits)
        fplan, bplan = _plans(d, C, G, res, biased, deferred)
        seen["fwd"].add(fplan.fwd)
        for k in ("bwd", "bits", "colsum"):
            seen[k].add(getattr(bplan, k))
    assert seen == {"fwd": set(FWD), "bwd": set(BWD), "bits": {False, True}, "colsum": {False, True}}
