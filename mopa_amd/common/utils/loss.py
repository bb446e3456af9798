"""Losses of the hot path as autograd nodes over libmopa_hip.so.

``mask_cons_loss`` keeps the reference signature (``mopa/common/utils/loss.py:241-283``);
``xm_kl`` / ``seg_ce`` / ``softmax_lastdim`` package the inline ``torch.nn.functional`` expressions of
``mopa/train/train_xmuda_mopa.py:354-363,389-398,472-473`` as single fused kernels.
Loss values, normalisers and the upstream gradient stay on the device (no host sync).
"""
from __future__ import annotations

from typing import List

import torch

from ..._lib import call, ptr, query, stream, workspace

import os as _os

VALIDATE_LABELS = _os.environ.get("MOPA_VALIDATE_LABELS", "0") == "1"   # host-syncing range checks (see seg_ce)


def _f32c(t):
    return t.contiguous().float()


class _SoftmaxKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit_p, logit_q):
        a, b = _f32c(logit_p), _f32c(logit_q.detach())
        N, C = a.shape
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        ws = workspace.get(query("mopa_loss_workspace_bytes", N), a.device)
        call("mopa_softmax_kl_fwd", ptr(a), ptr(b), N, C, ptr(loss), ptr(ws), ws.numel(), stream())
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = torch.empty_like(a)
        call("mopa_softmax_kl_bwd", ptr(a), ptr(b), a.shape[0], a.shape[1], ptr(_f32c(g)), ptr(da), stream())
        return da, None


def xm_kl(logit_p: torch.Tensor, logit_q: torch.Tensor) -> torch.Tensor:
    """F.kl_div(log_softmax(p), softmax(q.detach()), 'none').sum(1).mean()  (train_xmuda_mopa.py:389-398)."""
    # the target is detached BEFORE it enters the graph: as an input of the autograd node it would still schedule the other
    # network's backward (with zero gradients) -- a whole redundant backward pass per loss
    return _SoftmaxKL.apply(logit_p, logit_q.detach())


class _WeightedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index):
        z = _f32c(logits)
        y = labels.to(device=z.device, dtype=torch.int64).contiguous()
        w = None if weight is None else _f32c(weight.to(z.device))
        N, C = z.shape
        out = torch.empty(2, dtype=torch.float32, device=z.device)  # loss, normaliser
        status = torch.zeros(1, dtype=torch.int32, device=z.device)
        ws = workspace.get(query("mopa_loss_workspace_bytes", N), z.device)
        call("mopa_wce_fwd", ptr(z), ptr(y), ptr(w), N, C, ignore_index, ptr(out), ptr(out, 1), ptr(status), ptr(ws),
             ws.numel(), stream())
        ctx.save_for_backward(z, y, out)
        ctx.w, ctx.ignore_index, ctx.status = w, ignore_index, status
        if VALIDATE_LABELS and int(status.item()) != 0:   # a host sync: debugging / validation runs only
            raise IndexError(f"seg_ce: a label is outside [0, {C}) and is not ignore_index {ignore_index} "
                             "(F.cross_entropy raises 'Target out of bounds' here)")
        return out[0]

    @staticmethod
    def backward(ctx, g):
        z, y, out = ctx.saved_tensors
        dz = torch.empty_like(z)
        call("mopa_wce_bwd", ptr(z), ptr(y), ptr(ctx.w), z.shape[0], z.shape[1], ctx.ignore_index, ptr(out, 1),
             ptr(_f32c(g)), ptr(dz), stream())
        return dz, None, None, None


def seg_ce(logits, labels, weight=None, ignore_index: int = -100) -> torch.Tensor:
    """F.cross_entropy(logits, labels, weight=weight) with torch's default ignore_index (train_xmuda_mopa.py:354-363).

    Rows with label == ignore_index are skipped in-kernel, so the boolean-mask compaction the reference does
    for pseudo labels (:452-465, a device sync) is unnecessary: pass the full tensors.

    Deviation from ``F.cross_entropy``: a label outside ``[0, C)`` that is not ``ignore_index`` (e.g. 255, or a class-count
    mismatch) is dropped from numerator and normaliser instead of raising -- raising needs a device sync per call.  The kernel
    records the condition; set ``mopa_amd.common.utils.loss.VALIDATE_LABELS = True`` (or ``MOPA_VALIDATE_LABELS=1``) to check
    it after every call, e.g. for the first iterations of a new dataset.  The same switch validates SAM mask ids (> 255) in
    ``mask_cons_loss``.
    """
    if logits.shape[0] == 0:
        return logits.sum() * float("nan")
    return _WeightedCE.apply(logits, labels, weight, ignore_index)


class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        zc = _f32c(z)
        C = zc.shape[-1]
        p = torch.empty_like(zc)
        call("mopa_softmax_fwd", ptr(zc), zc.numel() // C, C, ptr(p), stream())
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, dp):
        p, = ctx.saved_tensors
        C = p.shape[-1]
        dz = torch.empty_like(p)
        call("mopa_softmax_bwd", ptr(p), ptr(_f32c(dp)), p.numel() // C, C, ptr(dz), stream())
        return dz


def softmax_lastdim(z: torch.Tensor) -> torch.Tensor:
    """F.softmax(z, dim=-1) (caller of mask_cons_loss: train_xmuda_mopa.py:473)."""
    return _Softmax.apply(z)


class _MaskCons(torch.autograd.Function):
    @staticmethod
    def forward(ctx, probs, masks, min_entropy):
        p = _f32c(probs)
        B, C = p.shape[0], p.shape[-1]
        HW = p.numel() // (B * C)
        k_norm = p.shape[1]  # quirk: the caller passes (B,H,W,C), so the normaliser is log2(H)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        state = torch.empty(query("mopa_mask_cons_state_floats", B, C), dtype=torch.float32, device=p.device)
        ws = workspace.get(query("mopa_mask_cons_workspace_bytes", B, HW, C), p.device)
        call("mopa_mask_cons_fwd", ptr(p), ptr(masks), B, HW, C, k_norm, int(min_entropy), ptr(loss), ptr(state),
             ptr(ws), ws.numel(), stream())
        ctx.save_for_backward(p, masks, state)
        ctx.args = (B, HW, C, k_norm, int(min_entropy))
        return loss

    @staticmethod
    def backward(ctx, g):
        p, masks, state = ctx.saved_tensors
        B, HW, C, k_norm, me = ctx.args
        dp = torch.empty_like(p)
        call("mopa_mask_cons_bwd", ptr(p), ptr(masks), B, HW, C, k_norm, me, ptr(state), ptr(_f32c(g)), ptr(dp), stream())
        return dp, None, None


def mask_cons_loss(all_logits: torch.Tensor, sam_mask_ls: List[torch.Tensor], min_entropy: bool = False):
    """Intra-mask consistency loss, same call as ``mopa/common/utils/loss.py:241``.

    ``all_logits``: per-pixel class probabilities as the caller passes them, (B,H,W,C)
    (``train_xmuda_mopa.py:473-478``); ``sam_mask_ls``: B tensors (H,W) of integer mask ids, negative = ignore,
    valid ids in [0,255] (uint8 SAM files).  Returns the mean over images of the mean over mask ids.
    """
    if len(sam_mask_ls) == 0:
        return 0
    dev = all_logits.device
    masks = torch.stack([torch.as_tensor(m).to(device=dev, dtype=torch.int32) for m in sam_mask_ls]).contiguous()
    if VALIDATE_LABELS and int(masks.max().item()) > 255:
        raise IndexError("mask_cons_loss: mask id > 255 (ids come from uint8 SAM files; larger ids would be treated as ignore)")
    if masks.shape[0] != all_logits.shape[0] or masks.numel() * all_logits.shape[-1] != all_logits.numel():
        raise RuntimeError(f"mask_cons_loss: probs {tuple(all_logits.shape)} vs masks {tuple(masks.shape)}")
    return _MaskCons.apply(all_logits, masks, bool(min_entropy))


# ------------------------------------------------------------------------------------------------ Lovasz-softmax (csrc/lovasz.hip)
LOVASZ_MAX_CLASSES = 64    # csrc/lovasz.hip: the selected classes of a segment are the bits of one word
LOVASZ_MAX_SEGMENTS = 32


def _lovasz_classes(classes, C):
    """-> (class_mode, class_mask) of mopa_lovasz_fwd."""
    if isinstance(classes, str):
        if classes not in ("present", "all"):
            raise ValueError(f"lovasz_softmax: classes must be 'present', 'all' or a list of classes, not {classes!r}")
        return (0 if classes == "present" else 1), 0
    mask = 0
    for c in classes:
        c = int(c)
        if not 0 <= c < C:
            raise ValueError(f"lovasz_softmax: class {c} of the list is outside [0, {C})")
        mask |= 1 << c
    return 2, mask


class _Lovasz(torch.autograd.Function):
    """loss (0-d float32) of contiguous float32 (P, C) probabilities or logits; backward = one mopa_lovasz_bwd launch."""

    @staticmethod
    def forward(ctx, x, labels, from_logits, offsets, ignore, mode, mask, aux):
        import ctypes
        P, C = x.shape
        dev = x.device
        S = len(offsets) - 1
        off = (ctypes.c_int64 * (S + 1))(*offsets)
        has_ignore = ignore is not None
        ign = int(ignore) if has_ignore else 0
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty((P, C), dtype=torch.float64 if from_logits else torch.float32, device=dev)
        lse = torch.empty(P, dtype=torch.float32, device=dev) if from_logits else None
        state = torch.empty(query("mopa_lovasz_state_bytes") // 8, dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ws = workspace.get(query("mopa_lovasz_workspace_bytes", P, C, S), dev)
        call("mopa_lovasz_fwd", ptr(x), int(from_logits), ptr(labels), P, C, ctypes.addressof(off), S, ign, int(has_ignore), mode, mask,
             ptr(loss), ptr(coef), ptr(lse), ptr(state), ptr(status), ptr(ws), ws.numel(), stream())
        ctx.save_for_backward(x, labels, coef, state)
        ctx.lse, ctx.args = lse, (bool(from_logits), tuple(offsets), ign, int(has_ignore))
        aux["state"], aux["status"] = state, status
        return loss

    @staticmethod
    def backward(ctx, g):
        import ctypes
        x, labels, coef, state = ctx.saved_tensors
        from_logits, offsets, ign, has_ignore = ctx.args
        P, C = x.shape
        S = len(offsets) - 1
        off = (ctypes.c_int64 * (S + 1))(*offsets)
        dx = torch.empty_like(x)
        call("mopa_lovasz_bwd", ptr(coef), int(from_logits), ptr(x), ptr(ctx.lse), ptr(labels), P, C, ctypes.addressof(off), S, ign,
             has_ignore, ptr(state), ptr(_f32c(g)), ptr(dx), stream())
        return dx, None, None, None, None, None, None, None


def _lovasz_call(name, x2d, labels, from_logits, offsets, ignore, classes):
    """x2d (P, C), labels (P,): checks, then the autograd node; the result carries .loss64 and .status."""
    P, C = x2d.shape
    if C == 1:
        raise ValueError(f"{name}: C == 1 (the reference's sigmoid branch) is not supported; the class dimension needs 2..64 entries")
    if not 2 <= C <= LOVASZ_MAX_CLASSES:
        raise ValueError(f"{name}: {C} classes are outside 2..{LOVASZ_MAX_CLASSES}")
    if labels.numel() != P:
        raise ValueError(f"{name}: {labels.numel()} labels for {P} rows of {tuple(x2d.shape)}")
    if not x2d.is_floating_point() or labels.is_floating_point():
        raise ValueError(f"{name}: floating-point probabilities and integer labels are expected")
    S = len(offsets) - 1
    if not 1 <= S <= LOVASZ_MAX_SEGMENTS:
        raise ValueError(f"{name}: {S} row segments are outside 1..{LOVASZ_MAX_SEGMENTS}")
    if offsets[0] != 0 or offsets[-1] != P or any(b < a for a, b in zip(offsets[:-1], offsets[1:])):
        raise ValueError(f"{name}: the segment offsets {list(offsets)} must rise from 0 to {P}")
    mode, mask = _lovasz_classes(classes, C)
    if not x2d.is_cuda:
        raise RuntimeError(f"{name}: the input is a CPU tensor; the hot path has no CPU fallback")
    if P == 0:   # nothing to sort: the zero the device gives when every row is ignored
        loss = x2d.sum() * 0.0
        loss.loss64 = torch.zeros((), dtype=torch.float64, device=x2d.device)
        loss.status = torch.zeros(1, dtype=torch.int32, device=x2d.device)
        return loss
    x = _f32c(x2d)
    y = labels.reshape(-1).to(device=x.device, dtype=torch.int64).contiguous()
    aux = {}
    loss = _Lovasz.apply(x, y, from_logits, [int(o) for o in offsets], ignore, mode, mask, aux)
    loss.status = aux["status"]
    loss.loss64 = aux["state"][0]
    if VALIDATE_LABELS and int(loss.status.item()) != 0:   # a host sync: debugging / validation runs only
        raise IndexError(f"{name}: a label is outside [0, {C}) and is not the ignore value {ignore}")
    return loss


def lovasz_softmax(probas, labels, classes='present', per_image=False, ignore=None) -> torch.Tensor:
    """Multi-class Lovasz-softmax loss, same call as ``mopa/common/utils/loss.py:122``: ``probas`` (P, C) or (B, C, H, W) class
    probabilities, ``labels`` (P,) or (B, H, W); ``classes``: 'present' (classes with a labelled row), 'all', or a list;
    ``per_image``: the mean of the per-image losses (the first dimension of a 4-D input; at most 32 images); ``ignore``: void label.

    One forward call of a fixed number of launches (a segmented radix sort per class, integer running counts, float64 Jaccard
    weights) and one backward launch; nothing is read back.  The result carries ``.loss64`` (0-d float64 tensor, the value before its
    one rounding to float32) and ``.status`` (int32 tensor: bit 0 a label outside [0, C) that is not ``ignore``).

    Deviations from the reference: equal errors keep ascending row order (``torch.sort`` leaves ties open);
    no valid row, or no selected class, gives 0 with a zero gradient (the reference returns a (0, C) tensor when every row is
    ignored and raises IndexError at exactly one valid row); a label outside [0, C) is foreground for no class and is recorded, not
    raised (``VALIDATE_LABELS`` checks after the call, as in ``seg_ce``); ``C == 1``, the sigmoid branch, raises ValueError."""
    if probas.dim() == 3:
        raise ValueError("lovasz_softmax: a (B, H, W) input is the reference's sigmoid branch (C == 1), which is not supported")
    if probas.dim() == 4:
        B, C, H, W = probas.shape
        x = probas.permute(0, 2, 3, 1).reshape(-1, C)   # one strided copy on the device; autograd routes the gradient back
        offsets = [b * H * W for b in range(B + 1)] if per_image else [0, B * H * W]
    elif probas.dim() == 2:
        if per_image:
            raise ValueError("lovasz_softmax: per_image=True needs a (B, C, H, W) input; for row segments of a (P, C) input use "
                             "lovasz_softmax_logits(..., segments=) or one call per segment")
        x, offsets = probas, [0, probas.shape[0]]
    else:
        raise ValueError(f"lovasz_softmax: probas must be (P, C) or (B, C, H, W), not {tuple(probas.shape)}")
    return _lovasz_call("lovasz_softmax", x, labels, False, offsets, ignore, classes)


class Lovasz_softmax(torch.nn.Module):
    """``mopa/common/utils/loss.py:191-199``: the module form of ``lovasz_softmax``."""

    def __init__(self, classes='present', per_image=False, ignore=None):
        super().__init__()
        self.classes, self.per_image, self.ignore = classes, per_image, ignore

    def forward(self, probas, labels):
        return lovasz_softmax(probas, labels, self.classes, self.per_image, self.ignore)


def lovasz_softmax_logits(logits, labels, classes='present', ignore_index: int = -100, segments=None) -> torch.Tensor:
    """``lovasz_softmax(softmax_lastdim(logits), labels, classes, ignore=ignore_index)`` for (P, C) logits without the (P, C)
    probability plane in memory: the kernels form p on the fly with the device function of ``softmax_lastdim`` (the same bits, so
    ``.loss64`` equals the two-step form's exactly) and the backward returns d loss / d logits, accumulated in float64 from float64
    coefficients and rounded once.  ``segments``: S + 1 row offsets (at most 32 segments, e.g. the scans of a merged batch): every
    segment is its own loss and the result is their mean, as ``per_image=True`` does for images."""
    if logits.dim() != 2:
        raise ValueError(f"lovasz_softmax_logits: logits must be (P, C), not {tuple(logits.shape)}")
    offsets = [0, logits.shape[0]] if segments is None else [int(o) for o in segments]
    return _lovasz_call("lovasz_softmax_logits", logits, labels, True, offsets, ignore_index, classes)


# -------------------------------------------------------------------------------------------------- l2_norm (csrc/supcon.hip)
L2_NORM_MAX_FEATURES = 128


class _L2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        N, F = x.shape
        y = torch.empty_like(x)
        norm = torch.empty(N, dtype=torch.float32, device=x.device)
        call("mopa_l2norm_rows_fwd", ptr(x), N, F, ptr(y), ptr(norm), stream())
        ctx.save_for_backward(y, norm)
        return y

    @staticmethod
    def backward(ctx, g):
        y, norm = ctx.saved_tensors
        dx = torch.empty_like(y)
        call("mopa_l2norm_rows_bwd", ptr(y), ptr(norm), ptr(_f32c(g)), y.shape[0], y.shape[1], ptr(dx), stream())
        return dx


def l2_norm(feats: torch.Tensor) -> torch.Tensor:
    """``feats / where(norm > 1e-8, norm, 1e-8)`` per row of ``feats (N, F)``, same call as ``mopa/common/utils/loss.py:230-238``, as
    one wavefront-per-row kernel each way (csrc/supcon.hip; 1 <= F <= 128).  The squares are summed in float64 and the norm rounded
    once to float32; the gradient is ``(g - y (y . g)) / norm`` where the norm is above 1e-8 and ``g / 1e-8`` where it is not (what
    autograd gives through the reference's ``torch.where``).  float16 / bfloat16 inputs are cast to float32 and get their gradient in
    their own dtype; the result is float32."""
    if feats.dim() != 2:
        raise ValueError(f"l2_norm: feats must be (N, F), not {tuple(feats.shape)}")
    N, F = feats.shape
    if not 1 <= F <= L2_NORM_MAX_FEATURES:
        raise ValueError(f"l2_norm: feature width {F} is outside 1..{L2_NORM_MAX_FEATURES}")
    if N == 0:
        raise ValueError("l2_norm: no rows")
    if not feats.is_floating_point():
        raise TypeError("l2_norm: feats must be a floating-point tensor")
    if not feats.is_cuda:
        raise RuntimeError("l2_norm: feats is a CPU tensor; the hot path has no CPU fallback")
    return _L2Norm.apply(feats.to(torch.float32).contiguous())
