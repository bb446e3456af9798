"""The eval forward of both networks without gradients, as one call: the EMA teacher pass of the MoPA iteration
(``mopa/train/train_xmuda_mopa.py:264-335``) and the predictor of ``validate()`` / ``test.py``.

``Teacher(model_2d, model_3d, ema_2d, ema_3d)`` runs the networks with the EMA weights IN PLACE: the parameters of the pass are
views into ``FlatEMA.shadow`` (built once from the optimizer's slices), the BatchNorm buffers are the student's live ones
(torch_ema averages parameters only).  Nothing of the student is read-modified: no copy of its flat buffer, no ``WEIGHTS_EPOCH``
bump, no ``Net2DSeg._calls``, no ``.eval()`` / ``.train()`` switch.  The derived weight forms of the shadow live in the teacher's
own dictionaries (``_lib.FormScope``; same kernels as the student's forms) keyed on ``FlatEMA.version``; the 3D native executor gets
its own holder.  With ``ema_* = None`` the live weights are used (validation): then the forms are the student's own.

The 2D backbone of a pass is recorded once per (B, H, W) into a command list and replayed by ``mopa_exec_replay``
(``dense2d.Graph2D.record_eval``): the first pass of a key runs eagerly, the second records, a ``RuntimeError`` while recording marks
the key eager for good, moved parameter / buffer / shadow addresses drop it.  Only the heads -- whose size follows the number of
points -- stay outside the list.

Deviations from the reference's loop: images of equal size go through ONE pass (``batched=True``; eval-mode BatchNorm uses the
running statistics, so an image's logits do not depend on its neighbours, but the convolution dispatcher may pick another algorithm
at another tile count: equal within the parity tolerance, not bit for bit; ``batched=False`` is the reference's one pass per image),
and the full-image head is only computed on request (``heads="all"``).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib, dense2d, pseudo, sparse3d
from ._lib import call, ptr, stream
from .models.xmuda_arch import Net2DSeg, _require_cuda

MAX_EVAL_KEYS = 8     # recorded (B, H, W) keys per Teacher; further shapes run eagerly
PACK_MAXB = 32        # images per mopa_pack_point_pix launch (csrc/ops2d.hip::PP_MAXB)


def group_by_size(sizes, batched=True):
    """[(H, W)] per image -> [[image positions]] of the passes: equal sizes together (in input order), first-seen size first;
    ``batched=False``: one pass per image."""
    if not batched:
        return [[i] for i in range(len(sizes))]
    groups = {}
    for i, s in enumerate(sizes):
        groups.setdefault(tuple(s), []).append(i)
    return list(groups.values())


def restore_order(groups, per_group_items):
    """Inverse of group_by_size: per_group_items[g][k] belongs to image groups[g][k] -> the items in input order."""
    n = sum(len(g) for g in groups)
    out = [None] * n
    for g, items in zip(groups, per_group_items):
        if len(items) != len(g):
            raise ValueError(f"restore_order: {len(items)} items for a group of {len(g)} images")
        for i, it in zip(g, items):
            out[i] = it
    return out


def _is_host(idx):
    return not (torch.is_tensor(idx) and idx.device.type == "cuda")


def pack_point_pix(img_indices, H, W, device):
    """Device-side ``Net2DSeg.pack_indices``: list of B (N_b, 2) int64 [row, col] DEVICE tensors -> (int32 pixel rows (sum N_b,),
    int32 status (1,): how many indices lay outside the H x W image -- those are clamped into it).  No host round trip."""
    ns = [int(t.shape[0]) for t in img_indices]
    idx = [t.reshape(-1, 2).to(torch.int64) for t in img_indices]
    total = sum(ns)
    pix = torch.empty(total, dtype=torch.int32, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)   # (the entry point clears it)
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    for s, e in _lib.chunk_ranges(len(idx), PACK_MAXB):
        n0, n = sum(ns[:s]), sum(ns[s:e])
        cat = idx[s].contiguous() if e - s == 1 else torch.cat(idx[s:e])
        off = np.concatenate([[0], np.cumsum(ns[s:e])]).astype(np.int64)
        st = status if s == 0 else torch.empty(1, dtype=torch.int32, device=device)
        call("mopa_pack_point_pix", ptr(cat), off.ctypes.data, e - s, H, W, ptr(pix, n0), ptr(st), stream())
        if s:   # later chunks number their images from 0: move them behind the earlier ones
            pix[n0:n0 + n] += s * Hp * Wp
            status += st
    return pix, status


def _image_list(img, what):
    if torch.is_tensor(img):
        if img.dim() != 4 or img.shape[1] != 3:
            raise RuntimeError(f"{what} must be (B,3,H,W), got {tuple(img.shape)}")
        return list(img.unbind(0)), img
    out = []
    for i, t in enumerate(img):
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 3 or t.shape[0] != 3:
            raise RuntimeError(f"{what}[{i}] must be (3,H,W), got {tuple(t.shape)}")
        out.append(t)
    if not out:
        raise ValueError(f"{what} is empty")
    return out, None


def plan_2d(batch, batched=True, prefer_ori=False):
    """The 2D passes of a batch, checked on the host before anything is enqueued -> (images, the (B,3,H,W) tensor they came as or
    None, index list or None, ready point_pix_2d or None, [(H, W)], groups of image positions, name of the index entry)."""
    names = (("ori_img", "ori_img_indices"), ("img", "img_indices"))
    for im_name, ix_name in names if prefer_ori else names[::-1]:
        if batch.get(im_name) is not None:
            break
    else:
        raise KeyError("Teacher: the batch holds neither `img` nor `ori_img`")
    imgs, whole = _image_list(batch[im_name], im_name)
    indices = batch.get(ix_name)
    pix_ready = batch.get("point_pix_2d") if im_name == "img" else None
    sizes = [(int(t.shape[1]), int(t.shape[2])) for t in imgs]
    groups = group_by_size(sizes, batched)
    if pix_ready is not None:
        if len(groups) != 1:
            raise ValueError("Teacher: `point_pix_2d` addresses the whole batch as one pass (equal image sizes, batched=True); "
                             "pass `img_indices` instead")
        return imgs, whole, None, pix_ready, sizes, groups, "point_pix_2d"
    if indices is None:
        raise KeyError(f"Teacher: `{im_name}` needs `{ix_name}` (or, with `img`, a ready `point_pix_2d`)")
    if len(indices) != len(imgs):
        raise IndexError(f"{ix_name} must hold one array per image: {len(indices)} for {len(imgs)} images")
    return imgs, whole, indices, None, sizes, groups, ix_name


class _Holder:
    """Where the 3D native executor keeps its per-network state for the teacher's weights (the student's lives on its own cache)."""


class _Branch:
    """One network of the pass: its tensors in ``spec.order`` -- parameters as views into the EMA shadow -- and its form scope."""

    def __init__(self, model, ema):
        self.model, self.ema = model, ema
        self.scope = _lib.FormScope(lambda: ("ema", ema.version)) if ema is not None else None
        self._src = self._flat = self._P = None

    def tensors(self):
        """-> (order, flat, P) of this pass."""
        order, live = self.model._cache.get(self.model)
        if self._src is not live or (self.ema is not None and self._shadow_ptr != self.ema.shadow.data_ptr()):
            flat = live
            if self.ema is not None:
                opt, shadow = self.ema.opt, self.ema.shadow
                slot = {id(p): sl for p, sl in zip(opt.params, opt._slices)}
                flat = []
                for t in live:
                    sl = slot.get(id(t))
                    # (a parameter the optimizer does not hold -- frozen -- has no average: the live tensor, as torch_ema leaves it)
                    flat.append(t if sl is None else shadow[sl[0]:sl[0] + sl[1]].view(t.shape))
                self._shadow_ptr = shadow.data_ptr()
            self._src, self._flat, self._P = live, flat, dict(zip(order, flat))
        return order, self._flat, self._P


class Teacher:
    """``predict(batch)`` / ``pseudo_labels(batch_trg, xm)``; see the module docstring.

    ``stats``: ``replays`` / ``recorded`` / ``eager`` / ``dropped`` passes of the 2D backbone, ``failed`` recordings."""

    def __init__(self, model_2d, model_3d, ema_2d=None, ema_3d=None, replay=True):
        for m in (model_2d, model_3d):   # the class counts of both passes, before the first of them runs
            if hasattr(m, "check_heads"):
                m.check_heads(width_too=False)
        self.b2, self.b3 = _Branch(model_2d, ema_2d), _Branch(model_3d, ema_3d)
        self.replay = bool(replay)
        self.graphs = {}
        self.holder3d = _Holder()
        self.dual = None
        self.stats = {"replays": 0, "recorded": 0, "eager": 0, "dropped": 0, "failed": 0}
        self.last_index_status = None   # (1,) int32 device tensor of the last predict: device-side indices outside their image (clamped)

    # ------------------------------------------------------------------------------------------------ 2D
    def _backbone(self, P, flat, imgc, dev):
        B, _, H, W = imgc.shape
        g = None
        if self.replay and (dense2d.GRAPH_2D or dense2d.NATIVE_2D) and dense2d.DEBUG is None:
            key = (B, H, W, stream(), dense2d.F4_ROLES, dense2d.NATIVE_2D and not dense2d.GRAPH_2D)
            g = self.graphs.get(key)
            if g is None and len(self.graphs) < MAX_EVAL_KEYS:
                g = self.graphs[key] = dense2d.Graph2D(B, H, W, dev)
            if g is not None and g.fwd is not None and g.params_moved(flat):   # a buffer, a parameter or the shadow moved
                del self.graphs[key]
                self.stats["dropped"] += 1
                g = None
            if g is not None and not g.failed:
                g.calls += 1
                if g.calls > 1:   # the first pass of a key runs eagerly and leaves every weight form and workspace behind
                    if g.fwd is None:
                        try:
                            g.record_eval(P, flat)
                            self.stats["recorded"] += 1
                        except RuntimeError:   # a weight form the eager pass did not leave, a refused host pointer, out of memory
                            g.failed, g.fwd = True, None
                            self.stats["failed"] += 1
                    if g.fwd is not None:
                        self.stats["replays"] += 1
                        return g.forward_eval(imgc)
        self.stats["eager"] += 1
        return dense2d._backbone_forward(P, imgc, False, 0.0, 0, None, dev, 1, keep_tape=False)[0]

    def _pass_2d(self, imgc, pix, want_all):
        """One pass of the 2D network on (B,3,H,W) -> (seg_logit, seg_logit2 or None, seg_logit_all or None)."""
        model = self.b2.model
        dev = imgc.device
        order, flat, P = self.b2.tensors()
        B, _, H, W = imgc.shape
        Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
        C, dual = model.num_classes, bool(model.dual_head)
        _lib.FORM_SCOPE = self.b2.scope
        try:
            with torch.cuda.device(dev):
                feat = self._backbone(P, flat, imgc, dev)
                pred_all = None
                if want_all:
                    pred_all = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
                    call("mopa_pixel_head_fwd", feat.p, feat.ld, B, Hp, Wp, H, W, 64, C, ptr(P["linear.weight"]), ptr(P["linear.bias"]),
                         ptr(pred_all), stream())
                N = pix.numel()
                l1 = torch.empty(N, C, dtype=torch.float32, device=dev)
                l2 = torch.empty(N, C, dtype=torch.float32, device=dev) if dual else None
                if N > 0:
                    feats = torch.empty(N, 64, dtype=torch.float32, device=dev)
                    call("mopa_output_layer_heads_fwd", feat.p, feat.ld, ptr(pix), N, 64, C, ptr(P["linear.weight"]), ptr(P["linear.bias"]),
                         ptr(P["linear2.weight"]) if dual else None, ptr(P["linear2.bias"]) if dual else None, ptr(feats), ptr(l1),
                         ptr(l2) if dual else None, stream())
        finally:
            _lib.FORM_SCOPE = None
        return l1, l2, pred_all

    def _predict_2d(self, plan, heads):
        dev = _require_cuda(self.b2.model)
        imgs, whole, indices, pix_ready, sizes, groups, ix_name = plan
        B = len(imgs)
        per_img, statuses = [], []
        for g in groups:
            H, W = sizes[g[0]]
            if whole is not None and len(g) == B:
                x = whole
            else:
                x = imgs[g[0]].unsqueeze(0) if len(g) == 1 else torch.stack([imgs[i] for i in g])
            x = x.to(dev, non_blocking=True).contiguous().float()
            if pix_ready is not None:    # (one pass over the whole batch: plan_2d made sure)
                l1, l2, pall = self._pass_2d(x, pix_ready.to(dev), heads == "all")
                break
            idx = [indices[i] for i in g]
            if any(_is_host(t) for t in idx):    # host-side index lists: the checked host packing, as in Net2DSeg.forward
                pix = Net2DSeg.pack_indices(idx, H, W, dev)
            else:
                pix, status = pack_point_pix(idx, H, W, dev)
                statuses.append(status)
                if os.environ.get("MOPA_VALIDATE_LABELS", "0") == "1":   # (a syncing check, like the label checks of the losses)
                    bad = int(status.item())
                    if bad:
                        raise IndexError(f"{ix_name}: {bad} indices outside the {H}x{W} image")
            l1, l2, pall = self._pass_2d(x, pix, heads == "all")
            if len(groups) > 1:
                ns = [int(np.asarray(t.shape if torch.is_tensor(t) else np.shape(t)).prod()) // 2 for t in idx]
                s1 = l1.split(ns)
                s2 = l2.split(ns) if l2 is not None else [None] * len(g)
                sa = pall.unbind(0) if pall is not None else [None] * len(g)
                per_img.append(list(zip(s1, s2, sa)))
        self.last_index_status = None if not statuses else statuses[0] if len(statuses) == 1 else torch.stack(statuses).sum(0)
        if len(groups) == 1:    # one pass in input order: the tensors as they are
            out = {"seg_logit_2d": l1}
            if l2 is not None:
                out["seg_logit2_2d"] = l2
            if heads == "all":
                out["seg_logit_all"] = pall
            return out
        items = restore_order(groups, per_img)
        out = {"seg_logit_2d": torch.cat([it[0] for it in items])}
        if items[0][1] is not None:
            out["seg_logit2_2d"] = torch.cat([it[1] for it in items])
        if heads == "all":   # one (B,H,W,C) tensor when the images share a size, else a list of (H,W,C)
            alls = [it[2] for it in items]
            out["seg_logit_all"] = torch.stack(alls) if len(set(sizes)) == 1 else alls
        return out

    # ------------------------------------------------------------------------------------------------ 3D
    def _predict_3d(self, batch, prefer_ori):
        model = self.b3.model
        dev = _require_cuda(model)
        names = ("ori_x", "x") if prefer_ori else ("x", "ori_x")
        x = next((batch[n] for n in names if batch.get(n) is not None), None)
        if x is None:
            raise KeyError("Teacher: the batch holds neither `x` nor `ori_x`")
        locs, feats = x[0], x[1]
        if model.net_3d.not_runnable:
            raise NotImplementedError(model.net_3d.not_runnable)
        geom = batch.get("geometry_3d")
        order, flat, P = self.b3.tensors()
        spec = model._spec()
        spec.native_holder = self.holder3d
        _lib.FORM_SCOPE = self.b3.scope
        try:
            with torch.cuda.device(dev):
                if geom is None:
                    geom = model.net_3d.geometry(locs)    # (the one host read-back of the pass)
                _, l1, l2 = sparse3d.SCNNetFunction.apply(spec, geom, False, feats.to(dev, non_blocking=True), *flat)
        finally:
            _lib.FORM_SCOPE = None
        out = {"seg_logit_3d": l1}
        if model.dual_head:
            out["seg_logit2_3d"] = l2
        return out

    # ------------------------------------------------------------------------------------------------ public
    @torch.no_grad()
    def predict(self, batch, heads="point", batched=True, prefer_ori=False):
        """-> {"seg_logit_2d", "seg_logit_3d"[, "seg_logit2_2d", "seg_logit2_3d"][, "seg_logit_all"]} (float32, per point in input
        order).  2D images: ``img`` (B,3,H,W) or a list of (3,H,W) of any sizes, else ``ori_img`` (``prefer_ori``: the other way
        round); their points: ``img_indices`` / ``ori_img_indices`` (list of (N_b,2) [row, col], host or device) or a ready
        ``point_pix_2d``.  3D: ``x`` or ``ori_x`` = [locs, feats], optionally ``geometry_3d``.  ``heads="all"`` adds the full-image
        logits: (B,H,W,C), or a list of (H,W,C) when the images differ in size."""
        if heads not in ("point", "all"):
            raise ValueError(f"heads must be 'point' or 'all', got {heads!r}")
        dev = _require_cuda(self.b2.model)
        _require_cuda(self.b3.model)
        plan = plan_2d(batch, batched, prefer_ori)
        from .step import DualStream
        if self.dual is None or self.dual.device != torch.device(dev):
            self.dual = DualStream(dev)
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream(dev)
            side = self.dual.side
            side.wait_stream(main)
            with torch.cuda.stream(side):     # the chain of short 3D launches first: it runs beside the 2D pass queued behind it
                out3 = self._predict_3d(batch, prefer_ori)
            out = self._predict_2d(plan, heads)
            main.wait_stream(side)
            for t in out3.values():           # allocated from the side stream's pool, read on the main stream from here on
                t.record_stream(main)
        out.update(out3)
        return out

    @torch.no_grad()
    def pseudo_labels(self, batch_trg, xm: bool, batched=True, ignore_label: int = -100):
        """The teacher block of the iteration (train_xmuda_mopa.py:264-332) -> (pseudo_label_2d, pseudo_label_3d), int64 device
        tensors compacted like the batch: by ``batch_trg["gather"]`` (scanprep.prepare_batch_3d) or by ``ori_keep_idx`` + ``ori_idxs``.
        Reads ``ori_img`` / ``ori_img_indices`` / ``ori_x`` where present."""
        out = self.predict(batch_trg, "point", batched, prefer_ori=True)
        ps2, ps3 = pseudo.pseudo_labels(out["seg_logit_2d"], out["seg_logit_3d"], bool(xm), ignore_label)
        gather = batch_trg.get("gather")
        if gather is None:
            gather = gather_index(batch_trg["ori_keep_idx"], batch_trg["ori_idxs"], ps2.device)
        ps2c = ps2.index_select(0, gather)
        return ps2c, (ps2c.clone() if xm else ps3.index_select(0, gather))


def gather_index(keep_idx, idxs, device):
    """``[keep][idxs]`` per scan of the concatenated per-point array as ONE index (int64, device), from the masks as the datasets
    store them: ``keep`` a boolean mask over the scan's points, ``idxs`` a boolean mask over the kept ones.  The size of the result
    is only known on the device: ONE read-back (``nonzero`` over the whole batch); ``scanprep``'s ``gather`` avoids it."""
    if len(keep_idx) != len(idxs):
        raise ValueError(f"ori_keep_idx holds {len(keep_idx)} scans, ori_idxs {len(idxs)}")
    masks = []
    for keep, idx in zip(keep_idx, idxs):
        keep, idx = torch.as_tensor(keep).to(device), torch.as_tensor(idx).to(device)
        if keep.dtype != torch.bool or idx.dtype != torch.bool:
            raise TypeError("ori_keep_idx and ori_idxs must hold boolean masks (over a scan's points / over the kept ones)")
        masks.append(torch.zeros_like(keep).masked_scatter_(keep, idx))    # the flags of the kept points, at the points' places
    if not masks:
        return torch.zeros(0, dtype=torch.int64, device=device)
    return torch.cat(masks).nonzero().reshape(-1)
