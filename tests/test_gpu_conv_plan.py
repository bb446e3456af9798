"""What ConvOp launches is what dense2d.conv_plan says, and it computes the convolution: forward, backward-data and weight gradient
against fp64 F.conv2d and its autograd, on the smallest shapes that reach every form (tile and block thresholds patched to 0).
Tolerances are those of tests/test_gpu_2d.py for the same kernels."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# 48 x 48 x 2 images: the smallest map with B H W >= F4_FWD_MIN_PIXELS; 48 x 52: a ragged tile column; 256 -> 256 at 16 x 24: F(2x2) forward
# (too few pixels for F(4x4)) with F(4x4) backward passes
SHAPES = [(64, 64, 2, 48, 48), (128, 64, 2, 48, 48), (64, 128, 2, 48, 52), (256, 256, 2, 16, 24)]
REACH = {"WINO4_DIRECT_MIN_TILES": 0, "WINO4_FUSED_MIN_BLOCKS": 0, "WINO4_WGRAD_FUSED_MIN_TILES": 0}
SETTINGS = [{}, {"WINO4_WGRAD_FUSED": False}, {"WINO4_CONV9": False}, {"WINO4_DIRECT": False}, {"F4_ROLES": ("dgrad", "wgrad")}, {"WINOGRAD": False}]


def _patches(setting):
    """The switches of a setting, with the thresholds at 0 so that these small shapes reach the one-kernel and fused forms -- except the
    fused GEMM + output transform's without the one-kernel convolution: there it stays as shipped and the plain F(4x4) form runs."""
    return {**{k: v for k, v in REACH.items() if not (k == "WINO4_FUSED_MIN_BLOCKS" and "WINO4_DIRECT" in setting)}, **setting}


CONV = {"direct": ["mopa_conv2d_igemm"], "F2": ["mopa_wino_input", "mopa_conv2d_igemm_batched", "mopa_wino_output"],
        "F4": ["mopa_wino4_input", "mopa_conv2d_igemm_batched", "mopa_wino4_output"], "F4 fused": ["mopa_wino4_input", "mopa_wino4_gemm_output"],
        "F4 one": ["mopa_wino4_conv"], "F4 one9": ["mopa_wino4_conv9"]}
WGRAD = {"direct": ["mopa_conv2d_bwd_weight"], "F2": ["mopa_wino_input", "mopa_wino_dout", "mopa_wino_bwd_weight"],
         "F4": ["mopa_wino4_input", "mopa_wino4_dout", "mopa_wino4_bwd_weight"], "F4 one": ["mopa_wino4_wgrad_fused"]}
# largest error over the largest reference element: the bounds of test_gpu_2d.py's weight-gradient tests for these kernels
# (test_transform_domain_weight_gradient_gemm_vs_fp64, test_wino4_one_kernel_weight_gradient_vs_fp64); the direct kernel: test_conv_fwd_dgrad_wgrad
DW_BOUND = {"F2": 1e-5, "F4": 3e-5, "F4 one": 2e-5}


def _nhwc(t):  # (B,C,H,W) cpu -> Img on cuda
    from mopa_amd.dense2d import Img
    B, C, H, W = t.shape
    return Img(t.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous().cuda(), B, H, W)


def _nchw(img):
    return img.dense().reshape(img.B, img.H, img.W, img.C).permute(0, 3, 1, 2).cpu()


def _close(got, ref, rtol=1e-4, atol=2e-5):
    ref = ref.detach().float().numpy() if torch.is_tensor(ref) else ref
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol * max(1.0, float(np.abs(ref).max())))


def _conv_ref(x, w, gout):
    """fp64 conv3x3 (padding 1) and its autograd: (out, dx, dw)."""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv2d(xr, wr, None, 1, 1)
    (ref * gout.double()).sum().backward()
    return ref.detach(), xr.grad, wr.grad


@functools.lru_cache(maxsize=None)
def _case(cin, cout, B, H, W):
    """Inputs and the fp64 reference of one shape, shared by every setting (never modified)."""
    rng = np.random.Generator(np.random.PCG64(cin + cout + W))
    x = torch.from_numpy(rng.standard_normal((B, cin, H, W), dtype=np.float32))
    w = torch.from_numpy(rng.standard_normal((cout, cin, 3, 3), dtype=np.float32) * 0.05)
    gout = torch.from_numpy(rng.standard_normal((B, cout, H, W), dtype=np.float32))
    return (x, w, gout) + _conv_ref(x, w, gout)


class _Recorder:
    """dense2d.call with the entry-point names written down (the weight-form kernels left out: they run once per weight version)."""

    def __init__(self, monkeypatch, dense2d):
        self.names, inner = [], dense2d.call

        def call(name, *args):
            if name.endswith("bwd_weight") or "weight" not in name:
                self.names.append(name)
            return inner(name, *args)
        monkeypatch.setattr(dense2d, "call", call)

    def take(self):
        got, self.names[:] = list(self.names), []
        return got


def _check_dw(dw, ref, form):
    if form == "direct":
        return _close(dw, ref, rtol=1e-3, atol=1e-4)
    err = float((dw.double().cpu() - ref).abs().max()) / float(ref.abs().max())
    print(f"dw ({form}): {err:.2e} of the largest element, bound {DW_BOUND[form]:.0e}")
    assert err < DW_BOUND[form], err


def _run(monkeypatch, dense2d, plan, op, xi, gout, refs, lazy=False):
    """ConvOp.forward(keep_v=True) + backward on xi: the launches are the plan's, the results the reference's."""
    ref, dx_ref, dw_ref = refs
    B, H, W = xi.B, xi.H, xi.W
    rec = _Recorder(monkeypatch, dense2d)
    transform = (lambda names: [n + "_bn" if n == "mopa_wino4_input" else n for n in names]) if lazy else (lambda names: names)
    out = dense2d.new_img(B, H, W, op.O, "cuda")
    V = op.forward(xi, out, keep_v=True)
    assert (V is not None) == plan.keeps_v
    assert rec.take() == transform(CONV[plan.fwd])
    _close(_nchw(out), ref, rtol=1e-4, atol=3e-5)
    for v in ((V, None) if V is not None else (None,)):   # as the network runs it, and as a caller without V does
        dx = dense2d.new_img(B, H, W, op.I, "cuda")
        dw = torch.full_like(op.w, float("nan"))
        op.backward(xi, _nhwc(gout), dx, dw, None, acc_dx=False, V=v)
        form = plan.wgrad if v is None else "F%d" % plan.wgrad_F   # (a V always goes to the two-operand form)
        assert rec.take() == (transform(WGRAD[form]) if v is None else WGRAD[form][1:]) + CONV[plan.dgrad]
        _close(_nchw(dx), dx_ref, rtol=1e-4, atol=3e-5)
        _check_dw(dw, dw_ref, form)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()).replace(" ", "") or "defaults")
@pytest.mark.parametrize("cin,cout,B,H,W", SHAPES)
def test_convop_runs_what_the_plan_says(cin, cout, B, H, W, setting, monkeypatch):
    from mopa_amd import dense2d
    for name, value in _patches(setting).items():
        monkeypatch.setattr(dense2d, name, value)
    x, w, gout, *refs = _case(cin, cout, B, H, W)
    plan = dense2d.conv_plan(cin, cout, 3, 1, 1, B, H, W, True)
    print(plan)
    _run(monkeypatch, dense2d, plan, dense2d.ConvOp(w.cuda(), None, 3, 1, 1), _nhwc(x), gout, refs)


def test_every_form_is_reached_by_the_cases_above(monkeypatch):
    """(A size computation: the shapes and settings above do reach each algorithm in each pass.)"""
    from mopa_amd import dense2d
    seen = {"fwd": set(), "wgrad": set(), "dgrad": set(), "keeps_v": set()}
    for setting in SETTINGS:
        with monkeypatch.context() as m:
            for name, value in _patches(setting).items():
                m.setattr(dense2d, name, value)
            for cin, cout, B, H, W in SHAPES:
                plan = dense2d.conv_plan(cin, cout, 3, 1, 1, B, H, W, True)
                for k in seen:
                    seen[k].add(getattr(plan, k))
    assert seen["fwd"] == set(CONV) and seen["dgrad"] == set(CONV) - {"F2"} and seen["wgrad"] == set(WGRAD) - {"F2"} and seen["keeps_v"] == {False, True}


def test_deferred_batchnorm_input_runs_where_the_plan_takes_it(monkeypatch):
    """A LazyImg (BatchNorm + ReLU applied on the way in) through a layer whose plan takes it: training forward and backward against the
    fp64 convolution of the materialised BatchNorm output; with MOPA_WINOGRAD=0 no layer takes one and ConvOp.forward says so."""
    from mopa_amd import dense2d
    for name, value in REACH.items():
        monkeypatch.setattr(dense2d, name, value)
    cin, cout, B, H, W = SHAPES[0]
    x, w, gout = _case(cin, cout, B, H, W)[:3]
    P = {"bn.weight": torch.linspace(0.5, 1.5, cin).cuda(), "bn.bias": torch.linspace(-1, 1, cin).cuda(),
         "bn.running_mean": torch.zeros(cin, device="cuda"), "bn.running_var": torch.ones(cin, device="cuda")}
    raw, y, stats = _nhwc(x), dense2d.new_img(B, H, W, cin, "cuda"), torch.empty(1, 4, cin, device="cuda")
    dense2d.bn_fwd_groups(raw, y, P, "bn", 1, None, True, stats, 1)
    plan = dense2d.conv_plan(cin, cout, 3, 1, 1, B, H, W, True)
    assert plan.takes_lazy
    op = dense2d.ConvOp(w.cuda(), None, 3, 1, 1)
    _run(monkeypatch, dense2d, plan, op, dense2d.LazyImg(raw, stats, 1), gout, _conv_ref(_nchw(y), w, gout), lazy=True)
    monkeypatch.setattr(dense2d, "WINOGRAD", False)
    assert not dense2d.conv_plan(cin, cout, 3, 1, 1, B, H, W, True).takes_lazy
    with pytest.raises(RuntimeError):
        op.forward(dense2d.LazyImg(raw, stats, 1), dense2d.new_img(B, H, W, cout, "cuda"), keep_v=True)
