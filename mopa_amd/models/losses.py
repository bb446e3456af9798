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
