"""The per-point loss-and-metric block of one domain half in one device pass (csrc/losses.hip: mopa_point_losses_fwd / _bwd).

``point_losses`` replaces, between the forward and backward passes of ``mopa/train/train_xmuda_mopa.py:353-418`` (source),
``:437-469`` (target) and ``:563-576`` (the VGI batch): the two ``F.cross_entropy`` calls, the two cross-modal ``F.kl_div`` calls,
the two ``SegIoU.update_dict`` calls and ``pc_mm_acc`` -- one forward launch pair for everything, one backward launch per network,
and no host read (``seg_ce`` x2 + ``xm_kl`` x2 are 8 forward and 4 backward launches, ``update_dict`` syncs the host twice per call).
Every scalar and every gradient has the bits ``seg_ce`` / ``xm_kl`` give on the same tensors.  The forward of mopa_point_losses_fwd is the
one-segment form of the merged block's kernels (one forward kernel set; its workspace is mopa_point_losses_seg_workspace_bytes(1));
the backward keeps a kernel of its own, which is faster on one segment (profiles/r33_trainloss_one_body.md).

The two networks keep separate autograd nodes, as the reference backpropagates ``sum(loss_2d)`` and ``sum(loss_3d)`` separately:
a node takes its own network's logits only, the other network's enter detached (see ``xm_kl``).

``point_losses_merged`` is the same block for a merged pass (source, target and the VGI batch as row segments of one logit tensor
per network; mopa_point_losses_seg_fwd / _seg_bwd), with the entropy of ``mopa/models/losses.py:21-34`` as a third per-segment term.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import call, ptr, query, stream, workspace
from .common.utils import loss as _loss


class PointLosses:
    """ce_2d, kl_2d, ce_3d, kl_3d: 0-d tensors with autograd (None where the term is absent); acc: int64[2] on the device
    (#masked rows predicted right, #masked rows) or None; status: int32[1], bit 0 = a label outside [0, C) that is not ignore_index."""
    __slots__ = ("ce_2d", "kl_2d", "ce_3d", "kl_3d", "acc", "status")

    def __init__(self):
        self.ce_2d = self.kl_2d = self.ce_3d = self.kl_3d = self.acc = self.status = None


class _Net:
    """What one network's node needs: its logits (detached, fp32, contiguous), the detached KL target, labels and the shared result."""

    def __init__(self, k, zm, zx, other, y, w, ignore_index, scalars):
        self.k, self.zm, self.zx, self.other, self.y, self.w, self.ignore_index, self.scalars = k, zm, zx, other, y, w, ignore_index, scalars


class _NetTerms(torch.autograd.Function):
    """(ce, kl) of one network from the shared forward result; backward = the one mopa_point_losses_bwd call of that network.
    `z_main` / `z_xm` are the network's own logits where they receive a gradient (None otherwise)."""

    @staticmethod
    def forward(ctx, net, z_main, z_xm):
        ctx.net = net
        ctx.dtypes = (None if z_main is None else z_main.dtype, None if z_xm is None else z_xm.dtype)
        sc, k = net.scalars, net.k
        return (sc[3 * k] if net.y is not None else None), (sc[3 * k + 2] if net.other is not None else None)

    @staticmethod
    def backward(ctx, g_ce, g_kl):
        net = ctx.net
        zm, zx = net.zm, net.zx
        ref = zm if zm is not None else zx
        N, C = ref.shape
        zero = None
        if g_ce is None or g_kl is None:
            zero = torch.zeros((), dtype=torch.float32, device=ref.device)
        g = torch.stack([(zero if g_ce is None else g_ce).float(), (zero if g_kl is None else g_kl).float()])
        has_ce, has_kl = net.y is not None, net.other is not None
        shared = has_kl and zx is zm
        dz_main = torch.empty_like(zm) if (has_ce or shared) else None
        dz_xm = dz_main if shared else (torch.empty_like(zx) if has_kl else None)
        call("mopa_point_losses_bwd", ptr(zm) if (has_ce or shared) else None, ptr(zx) if has_kl else None, ptr(net.other), ptr(net.y),
             ptr(net.w), N, C, net.ignore_index, ptr(net.scalars, 3 * net.k + 1), ptr(g), ptr(dz_main), ptr(dz_xm), stream())
        dm = dz_main if ctx.needs_input_grad[1] else None
        dx = dz_xm if ctx.needs_input_grad[2] else None
        if dm is not None and dm.dtype != ctx.dtypes[0]:
            dm = dm.to(ctx.dtypes[0])
        if dx is not None and dx.dtype != ctx.dtypes[1]:
            dx = dx.to(ctx.dtypes[1])
        return None, dm, dx


def _logits(preds, dual_head):
    """-> (main, xm) graph tensors of one network's output dict; xm is main without a dual head."""
    if preds is None:
        return None, None
    main = preds["seg_logit"]
    return main, (preds["seg_logit2"] if dual_head else main)


def _flat(t):
    d = t.detach()
    return d if (d.dtype == torch.float32 and d.is_contiguous()) else d.contiguous().float()


def point_losses(preds_2d, preds_3d, *, label=None, label_2d=None, label_3d=None, weight=None, kl=True, dual_head_2d=None,
                 ignore_index=-100, metric_2d=None, metric_3d=None, acc_mask=None, dual=None) -> PointLosses:
    """CE, cross-modal KL, SegIoU update and masked accuracy of one batch of points for both networks.

    preds_2d / preds_3d: the models' output dicts (``seg_logit`` (N, C), and ``seg_logit2`` when the head is dual), either may be None
    (the VGI batch has 3D only).  The 2D KL term trains ``seg_logit2`` when ``dual_head_2d`` (default: ``seg_logit2`` is in the dict), the
    3D one ``preds_3d['seg_logit2']`` when present; both compare with the other network's detached ``seg_logit``.
    label: (N,) labels of both networks (source half: ``seg_label``); label_2d / label_3d: one network's (target half: the pseudo
    labels; VGI batch: ``label_3d=cat_ps_label``).  A network without labels has no CE term and no metric update.
    weight: (C,) class weights of ``F.cross_entropy`` or None.  kl=False: no KL terms.
    metric_2d / metric_3d: ``SegIoU``; receive this batch's confusion matrix through ``add_matrix`` (no host sync).
    acc_mask: (N,) bool / uint8; ``.acc`` is then (#rows with the mask set whose 3D prediction equals label_3d, #rows with the mask set).
    dual: a ``mopa_amd.step.DualStream``; the 3D node is created on its side stream, so its backward -- and with it the whole 3D
    backward -- is queued there (``DualStream.on_side`` / ``backward_on_side``).

    The caller applies the lambdas to the returned scalars.  Labels outside [0, C) that are not ``ignore_index`` are dropped and
    flagged in ``.status``; ``MOPA_VALIDATE_LABELS=1`` reads it back and raises, as ``seg_ce`` does.  N == 0: nothing is launched,
    the terms are NaN (``F.cross_entropy`` / ``.mean()`` of nothing) and the metrics untouched.  CUDA tensors only."""
    if preds_2d is None and preds_3d is None:
        raise ValueError("point_losses: both preds_2d and preds_3d are None")
    if dual_head_2d is None or dual_head_2d is ...:
        dual_head_2d = preds_2d is not None and "seg_logit2" in preds_2d
    g2m, g2x = _logits(preds_2d, bool(dual_head_2d))
    g3m, g3x = _logits(preds_3d, preds_3d is not None and "seg_logit2" in preds_3d)
    ref = g2m if g2m is not None else g3m
    if not ref.is_cuda:
        raise RuntimeError("point_losses: the logits are CPU tensors; the hot path has no CPU fallback")
    dev = ref.device
    N, C = ref.shape
    for t in (g2m, g2x, g3m, g3x):
        if t is not None and (tuple(t.shape) != (N, C) or t.device != dev):
            raise RuntimeError(f"point_losses: logits of shape {tuple(t.shape)} on {t.device}, expected {(N, C)} on {dev}")
    y2 = label_2d if label_2d is not None else label
    y3 = label_3d if label_3d is not None else label
    y2 = None if (y2 is None or g2m is None) else y2
    y3 = None if (y3 is None or g3m is None) else y3
    has_kl = bool(kl) and g2m is not None and g3m is not None
    out = PointLosses()

    if N == 0:
        nan = float("nan")
        if y2 is not None:
            out.ce_2d = g2m.sum() * nan
        if y3 is not None:
            out.ce_3d = g3m.sum() * nan
        if has_kl:
            out.kl_2d, out.kl_3d = g2x.sum() * nan, g3x.sum() * nan
        if acc_mask is not None and y3 is not None:
            out.acc = torch.zeros(2, dtype=torch.int64, device=dev)
        out.status = torch.zeros(1, dtype=torch.int32, device=dev)
        return out

    def lab(y):
        if y is None:
            return None
        if y.numel() != N:
            raise RuntimeError(f"point_losses: {y.numel()} labels for {N} rows")
        return y.to(device=dev, dtype=torch.int64).contiguous()

    same = y2 is y3
    y2 = lab(y2)
    y3 = y2 if (same and y2 is not None) else lab(y3)
    w = None if weight is None else weight.to(dev).contiguous().float()
    if w is not None and w.numel() != C:
        raise RuntimeError(f"point_losses: {w.numel()} class weights for {C} classes")
    for m, y in ((metric_2d, y2), (metric_3d, y3)):
        if m is not None and y is not None and m.num_classes != C:
            raise ValueError(f"point_losses: a metric of {m.num_classes} classes for logits of {C}")
    want2, want3 = metric_2d is not None and y2 is not None, metric_3d is not None and y3 is not None
    mask = None
    if acc_mask is not None and y3 is not None:
        if acc_mask.numel() != N:
            raise RuntimeError(f"point_losses: acc_mask of {acc_mask.numel()} entries for {N} rows")
        mask = acc_mask.to(dev).contiguous()
        if mask.dtype != torch.uint8:
            mask = (mask if mask.dtype == torch.bool else mask.ne(0)).view(torch.uint8)

    z2m, z3m = (None if g2m is None else _flat(g2m)), (None if g3m is None else _flat(g3m))
    z2x = None if not has_kl else (z2m if g2x is g2m else _flat(g2x))
    z3x = None if not has_kl else (z3m if g3x is g3m else _flat(g3x))

    # one zero-filled int64 block: conf_2d | conf_3d | acc | status (the kernel adds to the first three and ORs into the last)
    ints = torch.zeros(2 * C * C + 3, dtype=torch.int64, device=dev)
    conf2, conf3 = ints[:C * C].view(C, C), ints[C * C:2 * C * C].view(C, C)
    acc = ints[2 * C * C:2 * C * C + 2]
    status = ints[2 * C * C + 2:].view(torch.int32)[:1]
    scalars = torch.empty(8, dtype=torch.float32, device=dev)
    ws = workspace.get(query("mopa_point_losses_workspace_bytes", N), dev)
    call("mopa_point_losses_fwd", ptr(z2m), ptr(z2x), ptr(z3m), ptr(z3x), ptr(y2), ptr(y3), ptr(w), N, C, ignore_index, ptr(scalars),
         ptr(conf2) if want2 else None, ptr(conf3) if want3 else None, ptr(mask), ptr(acc) if mask is not None else None, ptr(status),
         ptr(ws), ws.numel(), stream())
    out.status = status
    if mask is not None:
        out.acc = acc
    if want2:
        metric_2d.add_matrix(conf2)
    if want3:
        metric_3d.add_matrix(conf3)
    if _loss.VALIDATE_LABELS and int(status.item()) != 0:   # a host sync: debugging / validation runs only
        raise IndexError(f"point_losses: a label is outside [0, {C}) and is not ignore_index {ignore_index} "
                         "(F.cross_entropy raises 'Target out of bounds' here)")

    if y2 is not None or has_kl:
        net = _Net(0, z2m, z2x, z3m if has_kl else None, y2, w, ignore_index, scalars)
        shared = has_kl and z2x is z2m
        out.ce_2d, out.kl_2d = _NetTerms.apply(net, g2m if (y2 is not None or shared) else None, g2x if (has_kl and not shared) else None)
    if y3 is not None or has_kl:
        net = _Net(1, z3m, z3x, z2m if has_kl else None, y3, w, ignore_index, scalars)
        shared = has_kl and z3x is z3m
        args = (net, g3m if (y3 is not None or shared) else None, g3x if (has_kl and not shared) else None)
        if dual is not None:
            # the side stream waits for the fused forward; the node's backward reads these there
            with dual.on_side(z3m, z3x, z2m if has_kl else None, y3, w, scalars):
                out.ce_3d, out.kl_3d = _NetTerms.apply(*args)
        else:
            out.ce_3d, out.kl_3d = _NetTerms.apply(*args)
    return out


# ------------------------------------------------------------------------------------------------ a merged pass: row segments
MAX_SEGMENTS = 8   # PL_MAXSEG of csrc/losses.hip
_SEG_WORDS = 10    # int64 words of one descriptor: n, row0_2d, row0_3d, y_2d, y_3d, acc_mask, conf_2d, conf_3d, acc_out, flags
_FLAG_KL, _FLAG_WEIGHTED, _FLAG_MINENT = 1, 2, 4


class Segment:
    """One row segment of a merged pass: ``rows`` consecutive points of every network it takes part in (``in_2d`` / ``in_3d``; the
    VGI batch has ``in_2d=False``).  label / label_2d / label_3d, metric_2d / metric_3d and acc_mask as in ``point_losses``, for
    this segment's rows; weighted=False: its CE ignores the class weights (the target half's pseudo-label CE,
    train_xmuda_mopa.py:456-465); kl=False: no cross-modal terms; minent=True: the entropy of the main head's softmax
    (``entropy_loss``, mopa/models/losses.py:21-34) as ``ent_2d`` / ``ent_3d``."""
    __slots__ = ("rows", "label", "label_2d", "label_3d", "weighted", "kl", "minent", "in_2d", "in_3d", "metric_2d", "metric_3d", "acc_mask")

    def __init__(self, rows, *, label=None, label_2d=None, label_3d=None, weighted=True, kl=True, minent=False, in_2d=True, in_3d=True,
                 metric_2d=None, metric_3d=None, acc_mask=None):
        self.rows = int(rows)
        self.label, self.label_2d, self.label_3d = label, label_2d, label_3d
        self.weighted, self.kl, self.minent, self.in_2d, self.in_3d = bool(weighted), bool(kl), bool(minent), bool(in_2d), bool(in_3d)
        self.metric_2d, self.metric_3d, self.acc_mask = metric_2d, metric_3d, acc_mask


class SegmentLosses:
    """The terms of one segment: 0-d tensors with autograd, None where the term is absent; acc as ``PointLosses.acc``."""
    __slots__ = ("ce_2d", "kl_2d", "ent_2d", "ce_3d", "kl_3d", "ent_3d", "acc")

    def __init__(self):
        self.ce_2d = self.kl_2d = self.ent_2d = self.ce_3d = self.kl_3d = self.ent_3d = self.acc = None


class MergedLosses:
    """segments: one ``SegmentLosses`` per ``Segment``, in order; status: int32[1] shared by all segments (``PointLosses.status``)."""
    __slots__ = ("segments", "status")

    def __init__(self, segments, status):
        self.segments, self.status = segments, status


class _SegNet:
    """What one network's node of a merged pass needs.  `has`: per segment (ce, kl, ent) presence; `table`: the host descriptors,
    `keep`: the device tensors they point to."""

    def __init__(self, k, zm, zx, other, w, ignore_index, scalars, table, S, has, keep):
        self.k, self.zm, self.zx, self.other, self.w, self.ignore_index = k, zm, zx, other, w, ignore_index
        self.scalars, self.table, self.S, self.has, self.keep = scalars, table, S, has, keep


def _ptr0(t, dummy):
    """Device pointer, NULL for None; a tensor without elements (whose pointer may be NULL) gives a valid address nobody reads."""
    if t is None:
        return None
    return ptr(t) if t.numel() else ptr(dummy)


class _NetSegTerms(torch.autograd.Function):
    """(ce, kl, ent) x segments of one network from the shared forward result; backward = one torch.stack of the upstream scalars
    and the one mopa_point_losses_seg_bwd call of that network, which writes the gradient of the whole merged logit tensors."""

    @staticmethod
    def forward(ctx, net, z_main, z_xm):
        ctx.net = net
        ctx.dtypes = (None if z_main is None else z_main.dtype, None if z_xm is None else z_xm.dtype)
        sc, k = net.scalars, net.k
        out = []
        for s, (ce, kl, ent) in enumerate(net.has):
            b = 8 * s + 4 * k
            out += [sc[b] if ce else None, sc[b + 2] if kl else None, sc[b + 3] if ent else None]
        return tuple(out)

    @staticmethod
    def backward(ctx, *gs):
        net = ctx.net
        zm, zx = net.zm, net.zx
        N, C = zm.shape
        zero = None
        if any(g is None for g in gs):
            zero = torch.zeros((), dtype=torch.float32, device=zm.device)
        g = torch.stack([zero if t is None else t.float() for t in gs])
        has_kl = zx is not None
        shared = has_kl and zx is zm
        dz_main = torch.empty_like(zm)
        dz_xm = dz_main if shared else (torch.empty_like(zx) if has_kl else None)
        call("mopa_point_losses_seg_bwd", net.k, _ptr0(zm, g), _ptr0(zx, g), _ptr0(net.other, g), ptr(net.w), ctypes.addressof(net.table),
             net.S, N, 0 if net.other is None else net.other.shape[0], C, net.ignore_index, ptr(net.scalars), ptr(g), _ptr0(dz_main, g),
             _ptr0(dz_xm, g), stream())
        dm = dz_main if ctx.needs_input_grad[1] else None
        dx = dz_xm if ctx.needs_input_grad[2] else None
        if dm is not None and dm.dtype != ctx.dtypes[0]:
            dm = dm.to(ctx.dtypes[0])
        if dx is not None and dx.dtype != ctx.dtypes[1]:
            dx = dx.to(ctx.dtypes[1])
        return None, dm, dx


def point_losses_merged(preds_2d, preds_3d, segments, *, weight=None, dual_head_2d=None, ignore_index=-100, dual=None) -> MergedLosses:
    """``point_losses`` for every row segment of a merged pass (``step.merge_domains_2d`` / ``merge_domains_3d``: source, target and
    the VGI batch through each network at once) in ONE forward launch pair and one backward launch per network, whatever the number
    of segments; the backward writes the gradient of the whole merged ``seg_logit`` / ``seg_logit2`` (zeros on the rows of a segment
    without a term for that head) -- no slicing, no padding of slice gradients.

    preds_2d / preds_3d: the output dicts of the merged passes, either may be None.  segments: 1 .. 8 ``Segment``; a network's rows
    are the concatenation, in order, of the segments that take part in it, and their row counts must add up to its logits' rows.
    Each segment is reduced as ``point_losses`` reduces a call on its rows (same means, labels, class-weight use): its CE / KL values
    and, without ``minent``, its gradient rows have the bits of that call.  weight, dual_head_2d, ignore_index, dual: as in
    ``point_losses``.  A segment of 0 rows gives NaN terms.  CUDA tensors only."""
    segments = list(segments)
    if preds_2d is None and preds_3d is None:
        raise ValueError("point_losses_merged: both preds_2d and preds_3d are None")
    if not 1 <= len(segments) <= MAX_SEGMENTS:
        raise ValueError(f"point_losses_merged: {len(segments)} segments, 1 .. {MAX_SEGMENTS} are taken")
    if dual_head_2d is None or dual_head_2d is ...:
        dual_head_2d = preds_2d is not None and "seg_logit2" in preds_2d
    g2m, g2x = _logits(preds_2d, bool(dual_head_2d))
    g3m, g3x = _logits(preds_3d, preds_3d is not None and "seg_logit2" in preds_3d)
    ref = g2m if g2m is not None else g3m
    if ref.dim() != 2:
        raise ValueError(f"point_losses_merged: logits of shape {tuple(ref.shape)}, expected (N, C)")
    C = ref.shape[1]
    S = len(segments)
    ins = [(sg.in_2d and g2m is not None, sg.in_3d and g3m is not None) for sg in segments]
    for k, gm in enumerate((g2m, g3m)):
        if gm is None:
            continue
        if gm.dim() != 2 or gm.shape[1] != C:
            raise ValueError(f"point_losses_merged: logits of shape {tuple(gm.shape)}, expected (N, {C})")
        total = sum(sg.rows for sg, i in zip(segments, ins) if i[k])
        if total != gm.shape[0] or any(sg.rows < 0 for sg in segments):
            raise ValueError(f"point_losses_merged: the {2 + k}D segments hold {total} rows, the logits {gm.shape[0]}")
    if C < 2 and any(sg.minent for sg in segments):
        raise ValueError("point_losses_merged: minent needs at least two classes (the reference divides by log2(C))")
    if not ref.is_cuda:
        raise RuntimeError("point_losses_merged: the logits are CPU tensors; the hot path has no CPU fallback")
    dev = ref.device
    for gm, gx in ((g2m, g2x), (g3m, g3x)):
        if gm is not None and (gx.shape != gm.shape or gx.device != dev or gm.device != dev):
            raise RuntimeError(f"point_losses_merged: logits of shape {tuple(gx.shape)} on {gx.device}, expected {tuple(gm.shape)} on {dev}")
    w = None if weight is None else weight.to(dev).contiguous().float()
    if w is not None and w.numel() != C:
        raise RuntimeError(f"point_losses_merged: {w.numel()} class weights for {C} classes")

    def lab(y, n):
        if y.numel() != n:
            raise RuntimeError(f"point_losses_merged: {y.numel()} labels for a segment of {n} rows")
        return y.to(device=dev, dtype=torch.int64).contiguous()

    # per segment: labels, mask, flags; everything is checked before the one launch
    ys, masks, flags, has2, has3 = [], [], [], [], []
    for sg, (in2, in3) in zip(segments, ins):
        y2 = sg.label_2d if sg.label_2d is not None else sg.label
        y3 = sg.label_3d if sg.label_3d is not None else sg.label
        y2, y3 = (y2 if in2 else None), (y3 if in3 else None)
        same = y2 is y3
        y2 = None if y2 is None else lab(y2, sg.rows)
        y3 = y2 if (same and y2 is not None) else (None if y3 is None else lab(y3, sg.rows))
        for m, y in ((sg.metric_2d, y2), (sg.metric_3d, y3)):
            if m is not None and y is not None and m.num_classes != C:
                raise ValueError(f"point_losses_merged: a metric of {m.num_classes} classes for logits of {C}")
        mask = None
        if sg.acc_mask is not None and y3 is not None:
            if sg.acc_mask.numel() != sg.rows:
                raise RuntimeError(f"point_losses_merged: acc_mask of {sg.acc_mask.numel()} entries for a segment of {sg.rows} rows")
            mask = sg.acc_mask.to(dev).contiguous()
            if mask.dtype != torch.uint8:
                mask = (mask if mask.dtype == torch.bool else mask.ne(0)).view(torch.uint8)
        kl = sg.kl and in2 and in3
        ys.append((y2, y3))
        masks.append(mask)
        flags.append((_FLAG_KL if kl else 0) | (_FLAG_WEIGHTED if (sg.weighted and w is not None) else 0) | (_FLAG_MINENT if sg.minent else 0))
        has2.append((y2 is not None, kl, sg.minent and in2))
        has3.append((y3 is not None, kl, sg.minent and in3))
    any_kl = any(h[1] for h in has2)
    if not any(any(h) for h in has2 + has3):
        raise ValueError("point_losses_merged: no segment has a term")

    z2m, z3m = (None if g2m is None else _flat(g2m)), (None if g3m is None else _flat(g3m))
    z2x = None if not any_kl else (z2m if g2x is g2m else _flat(g2x))
    z3x = None if not any_kl else (z3m if g3x is g3m else _flat(g3x))

    # one zero-filled int64 block: per segment conf_2d | conf_3d | acc, then status
    per = 2 * C * C + 2
    ints = torch.zeros(S * per + 1, dtype=torch.int64, device=dev)
    status = ints[S * per:].view(torch.int32)[:1]
    scalars = torch.empty(S * 8, dtype=torch.float32, device=dev)
    table = (ctypes.c_int64 * (_SEG_WORDS * S))()
    row = [0, 0]
    out, confs = [], []
    for s, (sg, (in2, in3)) in enumerate(zip(segments, ins)):
        blk = ints[s * per:(s + 1) * per]
        conf2, conf3, acc = blk[:C * C].view(C, C), blk[C * C:2 * C * C].view(C, C), blk[2 * C * C:]
        y2, y3 = ys[s]
        want2, want3 = sg.metric_2d is not None and y2 is not None, sg.metric_3d is not None and y3 is not None
        words = (sg.rows, row[0] if in2 else -1, row[1] if in3 else -1, _ptr0(y2, scalars), _ptr0(y3, scalars), _ptr0(masks[s], scalars),
                 ptr(conf2) if want2 else None, ptr(conf3) if want3 else None, ptr(acc) if masks[s] is not None else None, flags[s])
        table[_SEG_WORDS * s:_SEG_WORDS * (s + 1)] = [0 if v is None else int(v) for v in words]
        row[0] += sg.rows if in2 else 0
        row[1] += sg.rows if in3 else 0
        res = SegmentLosses()
        if masks[s] is not None:
            res.acc = acc
        out.append(res)
        confs.append((conf2 if want2 else None, conf3 if want3 else None))
    ws = workspace.get(query("mopa_point_losses_seg_workspace_bytes", S), dev)
    call("mopa_point_losses_seg_fwd", _ptr0(z2m, scalars), _ptr0(z2x, scalars), _ptr0(z3m, scalars), _ptr0(z3x, scalars), ptr(w),
         ctypes.addressof(table), S, 0 if z2m is None else z2m.shape[0], 0 if z3m is None else z3m.shape[0], C, ignore_index, ptr(scalars),
         ptr(status), ptr(ws), ws.numel(), stream())
    for sg, (conf2, conf3) in zip(segments, confs):
        if conf2 is not None:
            sg.metric_2d.add_matrix(conf2)
        if conf3 is not None:
            sg.metric_3d.add_matrix(conf3)
    if _loss.VALIDATE_LABELS and int(status.item()) != 0:   # a host sync: debugging / validation runs only
        raise IndexError(f"point_losses_merged: a label is outside [0, {C}) and is not ignore_index {ignore_index} "
                         "(F.cross_entropy raises 'Target out of bounds' here)")

    keep = (ys, masks, ints)
    if z2m is not None and any(any(h) for h in has2):
        net = _SegNet(0, z2m, z2x, z3m if any_kl else None, w, ignore_index, scalars, table, S, has2, keep)
        shared = any_kl and z2x is z2m
        terms = _NetSegTerms.apply(net, g2m, g2x if (any_kl and not shared) else None)
        for s, res in enumerate(out):
            res.ce_2d, res.kl_2d, res.ent_2d = terms[3 * s:3 * s + 3]
    if z3m is not None and any(any(h) for h in has3):
        net = _SegNet(1, z3m, z3x, z2m if any_kl else None, w, ignore_index, scalars, table, S, has3, keep)
        shared = any_kl and z3x is z3m
        args = (net, g3m, g3x if (any_kl and not shared) else None)
        if dual is not None:
            # the side stream waits for the fused forward; the node's backward reads these there
            with dual.on_side(z3m, z3x, z2m if any_kl else None, w, scalars, ints, *[y for p in ys for y in p if y is not None]):
                terms = _NetSegTerms.apply(*args)
        else:
            terms = _NetSegTerms.apply(*args)
        for s, res in enumerate(out):
            res.ce_3d, res.kl_3d, res.ent_3d = terms[3 * s:3 * s + 3]
    return MergedLosses(out, status)
