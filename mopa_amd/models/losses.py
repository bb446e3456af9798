"""Losses of mopa/models/losses.py that run on the device.

``logcoral_loss`` (reference lines 47-93, ``TRAIN.XMUDA.lambda_logcoral``): the geodesic ("Deep logCORAL") distance between the
covariances of a source and a target feature batch, computed in float64 from the float32 features by csrc/coral.hip -- column means
and centred Gram matrices, a Jacobi eigendecomposition in LDS instead of the reference's SVD, the matrix logarithm, and in the
backward pass the divided-difference form of its derivative.  Everything is enqueued on the current stream;
nothing is read back (the reference synchronises the host for its guard, at least twice per call).
"""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import ptr

MAX_FEATURES = 64   # csrc/coral.hip: the F x F matrices of the eigen stage live in LDS

STATUS_GUARD, STATUS_NOT_CONVERGED, STATUS_NON_POSITIVE = 1, 2, 4


class _LogCoral(torch.autograd.Function):
    """loss (0-d float32) of two contiguous float32 (N, F) matrices; backward = one mopa_logcoral_bwd launch per input that needs a
    gradient."""

    @staticmethod
    def forward(ctx, xs, xt, batch_size, aux):
        F = xs.shape[1]
        dev = xs.device
        state = torch.empty(_lib.query("mopa_logcoral_state_bytes", F) // 8, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        nbytes = _lib.query("mopa_logcoral_workspace_bytes", F)
        ws = _lib.workspace.get(nbytes, dev)
        _lib.call("mopa_logcoral_fwd", ptr(xs), xs.shape[0], ptr(xt), xt.shape[0], F, batch_size, ptr(loss), ptr(state), ptr(status),
                  ptr(ws), ws.numel(), _lib.stream())
        ctx.save_for_backward(xs, xt)
        ctx.state, ctx.status = state, status
        aux["state"], aux["status"] = state, status
        return loss

    @staticmethod
    def backward(ctx, g):
        xs, xt = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        grads = []
        for side, x in enumerate((xs, xt)):
            if not ctx.needs_input_grad[side]:
                grads.append(None)
                continue
            dx = torch.empty_like(x)
            _lib.call("mopa_logcoral_bwd", ptr(x), x.shape[0], x.shape[1], side, ptr(ctx.state), ptr(ctx.status), ptr(g), ptr(dx),
                      _lib.stream())
            grads.append(dx)
        return grads[0], grads[1], None, None


def logcoral_loss(x_src: torch.Tensor, x_trg: torch.Tensor) -> torch.Tensor:
    """Geodesic (log-CORAL) loss between ``x_src (Ns, ..., F)`` and ``x_trg (Nt, ..., F)`` -> 0-d float32 tensor with autograd to both.

    The reference's quirks are kept: ``batch_size = x_src.shape[0]`` is read BEFORE the inputs are flattened to (N, F) and
    ``1 / (batch_size - 1)`` scales both covariances; a covariance entry > 1e30 or NaN on either side makes the loss exactly 0 with
    zero gradients.  Deviations: 1 <= F <= 64; fewer than two flattened rows on either side raise ValueError; where eigenvalues
    repeat, the gradient takes the limit of the divided difference (the reference's SVD backward gives 0/0).  On rank-deficient
    inputs (N <= F, a constant column) the result is log|lambda| under IEEE rules (-inf, then NaN in the products) as in the
    reference, and status bit 2 is set.

    The result carries ``.status`` (int32 tensor of one element on the device: bit 0 the guard fired, bit 1 the Jacobi iteration hit
    its sweep bound, bit 2 an eigenvalue was <= 0) and ``.loss64`` (0-d float64 view of the value before its rounding to float32).
    The call never reads either back."""
    if x_src.dim() < 2 or x_trg.dim() < 2:
        raise ValueError("logcoral_loss: the inputs need at least two dimensions (N, ..., F)")
    F = x_src.shape[-1]
    if x_trg.shape[-1] != F:
        raise ValueError(f"logcoral_loss: feature widths differ ({F} and {x_trg.shape[-1]})")
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError(f"logcoral_loss: feature width {F} is outside 1..{MAX_FEATURES} (the limit of the device eigen stage)")
    if not (x_src.is_floating_point() and x_trg.is_floating_point()):
        raise TypeError("logcoral_loss: the inputs must be floating-point tensors")
    batch_size = x_src.shape[0]
    if batch_size == 1:
        raise ZeroDivisionError("logcoral_loss: x_src.shape[0] == 1 (the reference divides by batch_size - 1)")
    if x_src.numel() // F < 2 or x_trg.numel() // F < 2:
        raise ValueError("logcoral_loss: fewer than two rows on one side (a covariance needs two)")
    if not (x_src.is_cuda and x_trg.is_cuda):
        raise RuntimeError("logcoral_loss: the features are CPU tensors; the hot path has no CPU fallback")
    if x_src.device != x_trg.device:
        raise ValueError("logcoral_loss: the inputs are on different devices")
    xs = x_src.reshape(-1, F).to(torch.float32).contiguous()
    xt = x_trg.reshape(-1, F).to(torch.float32).contiguous()
    aux = {}
    loss = _LogCoral.apply(xs, xt, batch_size, aux)
    loss.status = aux["status"]
    loss.loss64 = aux["state"][0]
    return loss


# ---------------------------------------------------------------------------------------- supervised contrastive (csrc/supcon.hip)
SUPCON_MAX_FEATURES = 128   # csrc/supcon.hip: SC_MAX_F


def supcon_tile_rows():
    """-> (anchor rows, pool rows) per tile of the kernels, as the library was compiled (SC_TA, SC_TQ of csrc/supcon.hip)."""
    return _lib.query("mopa_supcon_tile_rows", 0), _lib.query("mopa_supcon_tile_rows", 1)


SUPCON_NO_POSITIVE, SUPCON_NO_NEGATIVE, SUPCON_NON_FINITE = 1, 2, 4


class _SupCon(torch.autograd.Function):
    """loss (0-d float32) of contiguous float32 (Na, F) anchors and (Nq, F) pool features with int64 labels; backward = one
    mopa_supcon_bwd call per input that needs a gradient."""

    @staticmethod
    def forward(ctx, la, a, q, lq, T, skip_invalid, aux):
        Na, F = a.shape
        Nq = q.shape[0]
        dev = a.device
        state = torch.empty((_lib.query("mopa_supcon_state_bytes", Na) + 7) // 8, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = _lib.workspace.get(_lib.query("mopa_supcon_workspace_bytes", Na, Nq, F), dev)
        _lib.call("mopa_supcon_fwd", ptr(la), ptr(a), Na, ptr(q), ptr(lq), Nq, F, T, int(skip_invalid), ptr(loss), ptr(state), ptr(status),
                  ptr(ws), ws.numel(), _lib.stream())
        ctx.save_for_backward(la, a, q, lq)
        ctx.state, ctx.T = state, T
        aux["state"], aux["status"] = state, status
        return loss

    @staticmethod
    def backward(ctx, g):
        la, a, q, lq = ctx.saved_tensors
        Na, F = a.shape
        Nq = q.shape[0]
        g = g.to(torch.float32).contiguous()
        ws = _lib.workspace.get(_lib.query("mopa_supcon_workspace_bytes", Na, Nq, F), a.device)
        grads = []
        for side, x in ((0, a), (1, q)):
            if not ctx.needs_input_grad[1 + side]:
                grads.append(None)
                continue
            dx = torch.empty_like(x)
            _lib.call("mopa_supcon_bwd", ptr(la), ptr(a), Na, ptr(q), ptr(lq), Nq, F, ctx.T, side, ptr(ctx.state), ptr(g), ptr(dx),
                      ptr(ws), ws.numel(), _lib.stream())
            grads.append(dx)
        return None, grads[0], grads[1], None, None, None, None


def supcon_loss(labels_anchor: torch.Tensor, anchor_feature: torch.Tensor, contrast_feature: torch.Tensor, labels_contrast: torch.Tensor,
                temperature: float = 0.1, skip_invalid: bool = False) -> torch.Tensor:
    """The reference's class-wise contrastive loss (``SupConLoss.forward``, mopa/models/losses.py:131-184) between ``anchor_feature
    (Na, F)`` and the pool ``contrast_feature (Nq, F)`` -> 0-d float32 tensor with autograd to either or both feature tensors (the same
    tensor passed twice gets the sum of both gradients).  With ``S = A Q^T / temperature``: per anchor ``m = max_j S`` (held constant),
    ``D = sum over negatives of (exp(S - m) + float32(1e-5))`` -- only negatives enter the denominator, and there is no self-pair
    exclusion -- and ``loss = -mean_i ((1 / n_i) sum over positives of (S - m) - log D)``.  Nothing of size Na x Nq is allocated, on
    the device or here; nothing is read back.

    Deviations from the reference: an anchor without a positive (the reference's NaN assertion raises) or without a negative (the
    reference returns -inf with NaN gradients) is *invalid*: by default the loss is NaN and every gradient element NaN
    (``FlatAdam(skip_nonfinite=True)`` then skips the step); with ``skip_invalid=True`` such anchors are left out of the mean (none
    valid: exactly 0 with zero gradients).  Floating-point labels raise TypeError (``torch.eq`` would take them); 1 <= F <= 128.

    The result carries ``.status`` (int32 tensor of one element on the device: bit 0 an anchor has no positive, bit 1 an anchor has no
    negative, bit 2 a non-finite S was met) and ``.loss64`` (0-d float64 view of the value before its rounding to float32)."""
    a, q = anchor_feature, contrast_feature
    if a.dim() != 2 or q.dim() != 2:
        raise ValueError(f"supcon_loss: the features must be (N, F) matrices, not {tuple(a.shape)} and {tuple(q.shape)}")
    Na, F = a.shape
    Nq = q.shape[0]
    if q.shape[1] != F:
        raise ValueError(f"supcon_loss: feature widths differ ({F} and {q.shape[1]})")
    if not 1 <= F <= SUPCON_MAX_FEATURES:
        raise ValueError(f"supcon_loss: feature width {F} is outside 1..{SUPCON_MAX_FEATURES}")
    if Na == 0 or Nq == 0:
        raise ValueError(f"supcon_loss: no rows ({Na} anchors, {Nq} pool features)")
    if labels_anchor.numel() != Na or labels_contrast.numel() != Nq:
        raise ValueError(f"supcon_loss: {labels_anchor.numel()} / {labels_contrast.numel()} labels for {Na} anchors / {Nq} pool features")
    if not float(temperature) > 0.0:
        raise ValueError(f"supcon_loss: temperature {temperature} is not > 0")
    if not (a.is_floating_point() and q.is_floating_point()):
        raise TypeError("supcon_loss: the features must be floating-point tensors")
    if labels_anchor.is_floating_point() or labels_contrast.is_floating_point() or labels_anchor.is_complex() or labels_contrast.is_complex():
        raise TypeError("supcon_loss: the labels must be integer tensors (they are compared for equality only)")
    if not (a.is_cuda and q.is_cuda):
        raise RuntimeError("supcon_loss: the features are CPU tensors; the hot path has no CPU fallback")
    if a.device != q.device:
        raise ValueError("supcon_loss: the inputs are on different devices")
    af = a.to(torch.float32).contiguous()
    qf = af if q is a else q.to(torch.float32).contiguous()
    la = labels_anchor.reshape(-1).to(device=a.device, dtype=torch.int64).contiguous()
    lq = labels_contrast.reshape(-1).to(device=a.device, dtype=torch.int64).contiguous()
    aux = {}
    loss = _SupCon.apply(la, af, qf, lq, float(temperature), bool(skip_invalid), aux)
    loss.status = aux["status"]
    loss.loss64 = aux["state"][0]
    return loss


class SupConLoss(torch.nn.Module):
    """``mopa/models/losses.py:123-184``: the module form of ``supcon_loss``; ``iteration`` (the reference prints it when its NaN
    assertion fires) is accepted and unused."""

    def __init__(self, temperature=0.1, skip_invalid=False):
        super().__init__()
        self.temperature, self.skip_invalid = temperature, skip_invalid

    def forward(self, labels_anchor, anchor_feature, contrast_feature, labels_contrast, iteration=None):
        return supcon_loss(labels_anchor, anchor_feature, contrast_feature, labels_contrast, self.temperature, self.skip_invalid)
