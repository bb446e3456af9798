"""Flat-buffer optimizers (Adam, AdamW, SGD) + data-parallel gradient all-reduce.

All parameters of a network become views into ONE fp32 buffer and their ``.grad`` views into one flat gradient
buffer: one HIP launch updates the model (``mopa_adam_flat`` / ``mopa_adamw_flat`` / ``mopa_sgd_flat``) and the same flat buffer
is what RCCL all-reduces over xGMI -- one collective per network per iteration.  The reference builds its optimizer
as ``getattr(torch.optim, TYPE)`` (``mopa/common/solver/build.py:7-43``) and its config tree names ``Adam`` (yaml
``OPTIMIZER: TYPE Adam, BASE_LR 1e-3``) and ``SGD`` (``mopa/common/config/base.py:42-70``): ``FlatAdam``, ``FlatAdamW`` and
``FlatSGD`` have the semantics of the torch class of that name, and ``mopa_amd.common.solver.build.build_optimizer`` picks by
``TYPE``.  ``FlatOptimizer`` holds what the three share: the buffers, ``all_reduce()`` and the gradient buckets, ``grad_stats()`` and
the on-device clip / non-finite guard -- so ``FlatEMA``, ``Teacher`` and the bucketed backward work with any of them.

Each IS a ``torch.optim.Optimizer``: the reference hands its optimizer to ``build_scheduler`` (a
``MultiStepLR`` that rewrites ``param_groups[0]["lr"]``, ``mopa/common/solver/build.py:24-47``,
``train_xmuda_mopa.py:135-136``) and to ``CheckpointerV2`` which calls ``optimizer.state_dict()`` /
``load_state_dict()`` (``mopa/common/utils/checkpoint.py:48-49,76-77``).  ``state_dict()`` has exactly the layout of
the torch class (Adam / AdamW: per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq``; SGD: per-parameter ``momentum_buffer``; one
param group), so optimizer checkpoints move between the reference and this build in both directions.
"""
from __future__ import annotations

import math
import os

import torch
import torch.distributed as dist

from ._lib import GRAD_DONE_HOOKS, WEIGHTS_EPOCH, call, ptr, query, stream, workspace

# MOPA_FORCE_COLLECTIVES=1: issue the all-reduce in a one-rank process group too (exercises the RCCL path on a 1-GPU box)
_FORCE_COLLECTIVES = os.environ.get("MOPA_FORCE_COLLECTIVES") == "1"


class _Works:
    """Several asynchronous collectives behind the one `work.wait()` the callers use."""

    def __init__(self, works):
        self.works = works

    def wait(self):
        for w in self.works:
            w.wait()


def stat_chunks(slices, chunk):
    """The chunk table of ``mopa_grad_stats`` for ``FlatOptimizer._slices`` (``(offset, numel)`` per parameter): a list of
    ``(parameter index, lo, hi)`` ranges of the flat buffer, in parameter order.  Every parameter element is in exactly one
    chunk, no chunk crosses a parameter or touches the padding behind one, ``hi - lo <= chunk`` and ``lo % 4 == 0`` (the kernel
    reads a chunk as float4s from ``lo``)."""
    chunk = int(chunk)
    if chunk <= 0 or chunk % 4:
        raise ValueError("stat_chunks: the chunk length must be a positive multiple of 4")
    out = []
    for i, (off, n) in enumerate(slices):
        if off % 4:
            raise ValueError("stat_chunks: parameter %d starts at %d, not at a multiple of 4" % (i, off))
        out += [(i, lo, min(lo + chunk, off + n)) for lo in range(off, off + n, chunk)]
    return out


class GradStats:
    """What ``mopa_grad_stats`` left on the device for one gradient buffer -- tensors, no host read.  All norms are of
    ``grad_scale * g``.  The tensors are views of buffers the optimizer reuses: the next ``step()`` (for ``last_stats``) or
    ``grad_stats()`` call overwrites them (and returns this same object), so ``clone()`` what has to outlive it.

    ``norm`` () float32, ``nonfinite`` () int32: the whole buffer (a NaN / Inf element makes ``norm`` NaN / Inf, as torch's
    norm of norms does); ``param_norm`` / ``param_absmax`` (P,) float32 and ``param_nonfinite`` (P,) int32: per parameter, in
    the optimizer's parameter order (``param_absmax`` is over the finite elements).  After a guarded ``step()`` also ``coef`` ()
    float32 (the clip factor applied, 1 = not clipped), ``applied`` () int32 (0 = the step was skipped) and the running
    counters ``n_skipped`` / ``n_clipped`` () int64; ``None`` otherwise."""

    def __init__(self, norm, nonfinite, param_norm, param_absmax, param_nonfinite, coef=None, applied=None, n_skipped=None,
                 n_clipped=None):
        self.norm, self.nonfinite = norm, nonfinite
        self.param_norm, self.param_absmax, self.param_nonfinite = param_norm, param_absmax, param_nonfinite
        self.coef, self.applied, self.n_skipped, self.n_clipped = coef, applied, n_skipped, n_clipped

    def summary(self, names=None, top=5):
        """One line for the log.  The ONLY method here that reads back from the device (it synchronises): call it at the logging
        period, not every step.  Names the ``top`` parameters by norm and every parameter with non-finite entries; ``names``:
        one name per parameter (``[n for n, p in model.named_parameters() if p.requires_grad]``), default their indices."""
        pn, pnf = self.param_norm.detach().cpu(), self.param_nonfinite.detach().cpu()
        name = (lambda i: str(names[i])) if names is not None else (lambda i: "#%d" % i)
        parts = ["grad norm %.4g" % float(self.norm), "non-finite %d" % int(self.nonfinite)]
        if self.applied is not None:
            parts.append("coef %.4g, %s, skipped %d, clipped %d so far" % (float(self.coef), "applied" if int(self.applied) else "SKIPPED",
                                                                          int(self.n_skipped), int(self.n_clipped)))
        order = sorted(range(len(pn)), key=lambda i: -float(pn[i].nan_to_num(nan=float("inf"))))[:max(0, int(top))]
        if order:
            parts.append("largest: " + ", ".join("%s %.4g" % (name(i), float(pn[i])) for i in order))
        bad = [i for i in range(len(pnf)) if int(pnf[i]) > 0]
        if bad:
            parts.append("non-finite in: " + ", ".join("%s (%d)" % (name(i), int(pnf[i])) for i in bad))
        return "; ".join(parts)


class FlatOptimizer(torch.optim.Optimizer):
    """Everything about the flat buffers that is not one update rule: the parameters as views of ONE fp32 buffer ``flat`` and
    their ``.grad`` as views of ``grad``, the data-parallel ``all_reduce()`` and the gradient buckets, ``grad_stats()`` and the
    guard's step record, the ``step()`` convention.  A subclass gives
      * ``_NAME`` (what its messages call it),
      * ``_update(g, grad_scale, rec)``: enqueue the update kernel, behind the step record ``rec`` when that is not ``None``
        (``g`` is ``param_groups[0]``),
      * ``state_dict()`` / ``load_state_dict()`` in the layout of the torch optimizer it stands for."""
    _NAME = "FlatOptimizer"

    def __init__(self, params, defaults, checkpoint_shapes=None, max_grad_norm=None, skip_nonfinite=False):
        """``checkpoint_shapes``: optional list (one entry per parameter, ``None`` = the parameter's own shape) of the shapes
        the moment tensors take in ``state_dict()`` -- ``mopa_amd.models.scn_unet.checkpoint_shapes(model)`` gives
        SparseConvNet's 4-D conv-weight layout so that a reference-side ``torch.optim.Adam.load_state_dict`` of our
        checkpoint pairs every moment with a parameter of the same shape.

        ``max_grad_norm`` / ``skip_nonfinite`` (the guard; both off by default, and then ``step()`` is the single update launch
        it always was, ``mopa_adam_flat`` for ``FlatAdam``): with either set, ``step()`` first measures the gradient on the device
        (``mopa_grad_stats``: one read of the flat gradient, per-parameter and total 2-norm of ``grad_scale * g``, max |g|,
        non-finite count) and then runs the class's guarded kernel (``mopa_adam_flat_guarded``, ``mopa_adamw_flat_guarded``,
        ``mopa_sgd_flat_guarded``), which takes its decisions from device memory -- no host read, no sync.  ``max_grad_norm``: the
        update uses ``coef * grad_scale * g`` with ``coef = max_grad_norm / (norm + 1e-6)`` clamped to 1,
        ``torch.nn.utils.clip_grad_norm_``'s formula in float32 (norm type 2).  ``skip_nonfinite``: a step whose gradient holds a
        NaN or Inf writes nothing -- ``flat`` and the state buffers (``exp_avg`` / ``exp_avg_sq``, ``momentum_buf``) keep their
        bits.  ``last_stats`` holds the ``GradStats`` of the last guarded step.  Both are attributes of the optimizer, not
        ``param_groups`` entries: ``state_dict()`` keeps the torch optimizer's layout.  Differences from torch, on purpose, the
        same for every class:
          * ``p.grad`` is never modified (``clip_grad_norm_`` rewrites the gradients; here the factor goes into the update);
          * ``FlatAdam`` / ``FlatAdamW``: the step count ``t`` (bias corrections are host scalars) advances on a skipped step too --
            torch's fused Adam with ``found_inf`` rolls its device-side step back.  In exchange a guarded optimizer in which nothing
            triggers is bit-identical to the plain one, at the price of a bias correction a few steps ahead after a skip early in
            training.  (``FlatSGD`` has no step count; its "first step" rule follows the device: see the class);
          * there is no ``error_if_nonfinite`` (it needs a host sync): read ``last_stats.nonfinite`` at the logging period.
        Data parallel: ``step()`` runs after ``all_reduce()`` has been waited for, so every rank measures the same summed buffer
        -- a sum all-reduce leaves identical bits on all ranks -- and takes the same decision; no further collective."""
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("%s got no parameters" % self._NAME)
        if isinstance(params[0], dict):
            raise ValueError("%s takes one flat list of parameters (the reference builds a single param group)" % self._NAME)
        super().__init__(params, defaults)
        self.params = params
        dev = params[0].device
        sizes = [(p.numel() + 3) // 4 * 4 for p in params]  # keep every view 16-byte aligned
        self.n = sum(sizes)
        self.flat = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self._slices = []
        off = 0
        with torch.no_grad():
            for p, sz in zip(params, sizes):
                view = self.flat[off:off + p.numel()].view_as(p)
                view.copy_(p)
                p.data = view
                self._slices.append((off, p.numel()))
                off += sz
        self._attach_grads()
        self.n_collectives = 0        # all-reduces issued so far, and the backend of the last one (bench.py / tests report them)
        self.collective_backend = None
        self._ckpt_shapes = list(checkpoint_shapes) if checkpoint_shapes is not None else [None] * len(params)
        if len(self._ckpt_shapes) != len(params):
            raise ValueError("checkpoint_shapes must have one entry per trainable parameter")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("%s: max_grad_norm must be positive (None = no clipping)" % self._NAME)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.last_stats = None        # GradStats of the last guarded step()
        self._gs = None               # device side of mopa_grad_stats: built on first use

    # ---- reference-facing conveniences (kept from round 1)
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v):
        self.param_groups[0]["lr"] = v

    def _grad_view(self, i):
        off, n = self._slices[i]
        return self.grad[off:off + n].view_as(self.params[i])

    def _attach_grads(self):
        self._gviews = [self._grad_view(i) for i in range(len(self.params))]
        for p, g in zip(self.params, self._gviews):
            p.grad = g

    def _check_grads(self):
        """Every ``p.grad`` must still be the view of the flat gradient buffer the HIP kernels accumulate into.
        ``model.zero_grad()`` (torch's default sets grads to None) or a hook that replaces ``.grad`` would otherwise make
        ``step`` and ``all_reduce`` read a stale flat buffer without any error.  A detached slice is STALE -- whoever dropped
        the view meant "zero", and nothing has accumulated into the slice since -- so the parameter's own ``.grad`` is the
        truth: its value replaces the slice (``None`` = no gradient this iteration = zeros), and the view is re-attached."""
        for i, (p, gv) in enumerate(zip(self.params, self._gviews)):
            g = p.grad
            if g is gv:      # autograd accumulates in place: the tensor object we attached is still the gradient (~0.1 us per check)
                continue
            view = self._gviews[i] = self._grad_view(i)
            if g is None:
                view.zero_()
            else:               # autograd attached a fresh tensor after the view was dropped: it holds everything accumulated since
                if g.shape != p.shape:
                    raise RuntimeError("%s: a parameter's .grad was replaced by a tensor of another shape" % self._NAME)
                view.copy_(g)
            p.grad = view

    def zero_grad(self, set_to_none: bool = False):
        """In-place memset; the ``.grad`` views stay attached so the backward kernels accumulate into the flat buffer
        (``set_to_none`` is accepted for API compatibility and ignored: dropping the views would break that)."""
        self.grad.zero_()
        self._checked = False

    def _collectives_on(self):
        return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or _FORCE_COLLECTIVES)

    def all_reduce(self, async_op=False):
        """Sum the flat gradient over ranks (RCCL when the process group backend is 'nccl').  With armed buckets (enable_buckets +
        arm_buckets): the buckets whose all-reduce the backward pass has issued already are only waited for (the current stream
        waits for the communication stream; the host does not block), the others are issued now."""
        if not self._collectives_on():
            return None
        self._check_grads()
        self._checked = True   # once per iteration (~0.1 ms of host time for 200 parameters)
        self.collective_backend = dist.get_backend()
        if self._armed:
            for b in range(len(self._buckets)):
                if not self._bucket_issued[b]:
                    self._issue_bucket(b)
            self._armed = False
            cur = torch.cuda.current_stream(self.grad.device) if self.grad.is_cuda else None
            works, self._bucket_works = self._bucket_works, []
            if async_op:
                return _Works(works)
            for w in works:
                w.wait()
            if cur is not None and self._comm is not None:
                cur.wait_stream(self._comm)
            return None
        self.n_collectives += 1
        return dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, async_op=async_op)

    # ---- gradient buckets: the flat buffer cut into contiguous ranges in BACKWARD order, each all-reduced as soon as the backward
    # pass has enqueued the last kernel that writes into it -- the collective of the layers that finish first (decoder, layer4)
    # runs on a communication stream under the rest of the backward pass.  One flat buffer stays the optimizer's view.
    _armed = False
    _buckets = ()
    _comm = None

    def enable_buckets(self, n_buckets=4, extra_streams=None):
        """Cut the flat gradient buffer into `n_buckets` contiguous ranges of about equal size; bucket 0 holds the LAST parameters
        (their gradients are final first).  `extra_streams`: callable -> streams besides the current one that gradient kernels
        run on (the 2D weight-gradient stream); a bucket's collective is ordered behind all of them.  Takes effect for a
        backward pass only after arm_buckets()."""
        n_par = len(self.params)
        target = self.n / max(1, n_buckets)
        cuts, acc = [n_par], 0
        for i in range(n_par - 1, -1, -1):     # walk the parameters in backward order
            acc += self._slices[i][1]
            if acc >= target and len(cuts) < n_buckets and i > 0:
                cuts.append(i)
                acc = 0
        cuts.append(0)
        self._buckets = []                     # (first parameter, one past the last, flat offset lo, hi)
        for hi_p, lo_p in zip(cuts[:-1], cuts[1:]):
            if lo_p == hi_p:
                continue
            lo = self._slices[lo_p][0]
            hi = self.n if hi_p == n_par else self._slices[hi_p][0]
            self._buckets.append((lo_p, hi_p, lo, hi))
        self._bucket_of = {}                   # id(parameter) -> (bucket, parameter index)
        for b, (lo_p, hi_p, _, _) in enumerate(self._buckets):
            for i in range(lo_p, hi_p):
                self._bucket_of[id(self.params[i])] = (b, i)
        self._extra_streams = extra_streams
        self._comm = torch.cuda.Stream(device=self.grad.device) if self.grad.is_cuda else None
        self._bucket_works, self._bucket_issued, self._bucket_left = [], [False] * len(self._buckets), [0] * len(self._buckets)
        return [(hi - lo) * 4 for _, _, lo, hi in self._buckets]

    def disable_buckets(self):
        """Back to one collective per iteration; drops this optimizer's entries from the GradSink hook table."""
        for p in self.params:
            if GRAD_DONE_HOOKS.get(id(p)) == self._grad_done:
                del GRAD_DONE_HOOKS[id(p)]
        self._buckets, self._armed = (), False

    def arm_buckets(self):
        """Call right before the LAST backward pass of the iteration (gradients of earlier passes accumulate first: the reference
        runs the source and the target half before the optimizer step, train_xmuda_mopa.py:342-427)."""
        if not self._buckets or not self._collectives_on():
            return False
        if os.environ.get("MOPA_DIRECT_GRADS", "1") == "0":
            # without in-place gradients autograd's AccumulateGrad adds a pass's gradients to .grad only AFTER Function.backward has
            # returned -- after the bucket's all-reduce would have been enqueued: the collective would race with that add
            raise RuntimeError("%s.arm_buckets needs the gradients written in place (MOPA_DIRECT_GRADS=0 is set): "
                               "use all_reduce() after backward instead" % self._NAME)
        self._check_grads()
        self._checked = True
        self._armed = True
        self._bucket_works = []
        self._bucket_issued = [False] * len(self._buckets)
        self._bucket_left = [hi_p - lo_p for lo_p, hi_p, _, _ in self._buckets]
        self._done_ids = set()
        for p in self.params:
            GRAD_DONE_HOOKS[id(p)] = self._grad_done
        return True

    def _grad_done(self, p, final=False):
        """GradSink: the kernels writing p's gradient in this backward pass are enqueued (reported once per parameter: a parameter
        two kernels write -- the 2D head's point and pixel parts -- is reported after the first; its bucket also holds the decoder
        layers that follow both in stream order, and a bucket that went out before a late writer is refused below)."""
        if not self._armed:
            return
        b, i = self._bucket_of.get(id(p), (None, None))
        if b is None or self.params[i] is not p:   # (an id re-issued to another tensor after this optimizer's parameter died)
            return
        if id(p) in self._done_ids:
            if self._bucket_issued[b] and not final:
                raise RuntimeError("%s buckets: a gradient was written after its bucket's all-reduce had been issued" % self._NAME)
            return
        self._done_ids.add(id(p))
        self._bucket_left[b] -= 1
        # buckets go out in order (every rank issues the same sequence of collectives): bucket b only once b - 1 is out
        while b < len(self._buckets) and self._bucket_left[b] <= 0 and not self._bucket_issued[b] and (b == 0 or self._bucket_issued[b - 1]):
            self._issue_bucket(b)
            b += 1

    def _issue_bucket(self, b):
        _, _, lo, hi = self._buckets[b]
        self._bucket_issued[b] = True
        self.n_collectives += 1
        self.collective_backend = dist.get_backend()
        view = self.grad[lo:hi]
        if self._comm is None:
            self._bucket_works.append(dist.all_reduce(view, op=dist.ReduceOp.SUM, async_op=True))
            return
        self._comm.wait_stream(torch.cuda.current_stream(self.grad.device))
        for st in (self._extra_streams() if self._extra_streams is not None else ()):
            if st is not None:
                self._comm.wait_stream(st)
        with torch.cuda.stream(self._comm):
            self._bucket_works.append(dist.all_reduce(view, op=dist.ReduceOp.SUM, async_op=True))

    # ---- gradient statistics and the guarded step (csrc/optim.hip)
    def _grad_stats(self, grad_scale, max_norm, skip_nonfinite, which):
        if self.flat.device.type != "cuda":
            raise RuntimeError("%s gradient statistics need the HIP extension on an MI355X (no CPU fallback)" % self._NAME)
        if self._gs is None:    # once: the chunk table goes up; a (stats, step record) pair and its views for step(), one for grad_stats()
            dev, n_par = self.grad.device, len(self.params)
            tab = torch.tensor(stat_chunks(self._slices, query("mopa_grad_stats_chunk")), dtype=torch.int64).reshape(-1, 3)
            self._gs = {"tab": tab.to(dev), "n_chunks": int(tab.shape[0]),
                        "ws_bytes": query("mopa_grad_stats_workspace_bytes", int(tab.shape[0]))}
            for which_ in ("step", "query"):
                stats = torch.zeros(3, n_par, dtype=torch.float32, device=dev)
                rec = torch.zeros(8, dtype=torch.int32, device=dev)   # csrc/optim.hip::GsStepRec; the counters start at 0
                out = GradStats(rec[0:1].view(torch.float32)[0], rec[1], stats[0], stats[1], stats[2].view(torch.int32))
                if which_ == "step":
                    counters = rec[4:8].view(torch.int64)
                    out.coef, out.applied, out.n_skipped, out.n_clipped = rec[2:3].view(torch.float32)[0], rec[3], counters[0], counters[1]
                self._gs[which_] = (stats, rec, out)
        gs = self._gs
        stats, rec, out = gs[which]
        ws = workspace.get(gs["ws_bytes"], self.grad.device)
        call("mopa_grad_stats", ptr(self.grad), ptr(gs["tab"]), gs["n_chunks"], len(self.params), grad_scale, max_norm,
             int(skip_nonfinite), ptr(stats), ptr(rec), ptr(ws), gs["ws_bytes"], stream())
        return out, rec

    @torch.no_grad()
    def grad_stats(self, grad_scale: float = 1.0) -> GradStats:
        """Measure the flat gradient as it stands (after backward / ``all_reduce()``), with or without the guard: enqueues
        ``mopa_grad_stats`` on the current stream and returns device tensors -- no sync.  Touches neither ``last_stats`` nor the
        guard's counters."""
        if not getattr(self, "_checked", False):
            self._check_grads()
        return self._grad_stats(grad_scale, 0.0, False, "query")[0]

    @torch.no_grad()
    def step(self, grad_scale: float = 1.0, closure=None):
        """``step()`` / ``step(grad_scale)`` / ``step(closure)``: torch's convention puts the closure first, so a callable in
        the first position is taken as the closure.  ``grad_scale`` multiplies the gradient inside the update kernel
        (``1 / world_size`` after a sum all-reduce, times the rank's loss weight)."""
        if callable(grad_scale):
            closure, grad_scale = grad_scale, 1.0
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        else:
            loss = None
        if not getattr(self, "_checked", False):
            self._check_grads()
        self._checked = False
        if self.flat.device.type != "cuda":
            raise RuntimeError("%s.step needs the HIP extension on an MI355X (no CPU fallback)" % self._NAME)
        g = self.param_groups[0]
        if self.max_grad_norm is None and not self.skip_nonfinite:
            self._update(g, grad_scale, None)
        else:
            self.last_stats, rec = self._grad_stats(grad_scale, self.max_grad_norm or 0.0, self.skip_nonfinite, "step")
            self._update(g, grad_scale, rec)
        WEIGHTS_EPOCH[0] += 1   # cached weight re-layouts (dense2d / sparse3d) are stale now (a skipped step rebuilds them unchanged)
        return loss

    def _update(self, g, grad_scale, rec):
        raise NotImplementedError

    def _state_groups(self):
        groups = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        groups[0]["params"] = list(range(len(self.params)))
        return groups

    def _load_groups(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError("%s.load_state_dict: expected one param group with %d parameters" % (self._NAME, len(self.params)))
        for k, v in groups[0].items():
            if k != "params":
                self.param_groups[0][k] = tuple(v) if k == "betas" else v


class FlatAdam(FlatOptimizer):
    """``torch.optim.Adam`` on the flat buffers (``mopa_adam_flat`` / ``mopa_adam_flat_guarded``); the constructor's arguments
    beyond torch's are ``FlatOptimizer``'s."""
    _NAME = "FlatAdam"
    _KERNEL = "mopa_adam_flat"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, checkpoint_shapes=None,
                 max_grad_norm=None, skip_nonfinite=False):
        super().__init__(params, self._defaults(lr, betas, eps, weight_decay), checkpoint_shapes, max_grad_norm, skip_nonfinite)
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.t = 0

    @staticmethod
    def _defaults(lr, betas, eps, weight_decay):
        return dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False)

    def _update(self, g, grad_scale, rec):
        b1, b2 = g["betas"]
        self.t += 1             # on a skipped step too (the bias corrections are host scalars): see FlatOptimizer.__init__
        args = (ptr(self.flat), ptr(self.grad), ptr(self.exp_avg), ptr(self.exp_avg_sq), self.n, float(g["lr"]), b1, b2, g["eps"],
                g["weight_decay"], 1.0 - b1 ** self.t, math.sqrt(1.0 - b2 ** self.t), grad_scale)
        if rec is None:
            call(self._KERNEL, *args, stream())
        else:
            call(self._KERNEL + "_guarded", *args, ptr(rec), stream())

    # ---- checkpointing in torch.optim.Adam's layout (mopa/common/utils/checkpoint.py:48-49,76-77)
    def state_dict(self):
        state = {}
        if self.t > 0:
            for i, (off, n) in enumerate(self._slices):
                shape = self._ckpt_shapes[i] or self.params[i].shape
                state[i] = {"step": torch.tensor(float(self.t)),
                            "exp_avg": self.exp_avg[off:off + n].view(shape).clone(),
                            "exp_avg_sq": self.exp_avg_sq[off:off + n].view(shape).clone()}
        return {"state": state, "param_groups": self._state_groups()}

    def load_state_dict(self, sd):
        self._load_groups(sd)
        steps = set()
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for key, st in sd["state"].items():
            i = int(key)
            off, n = self._slices[i]
            self.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError("%s.load_state_dict: parameters with different step counts (one fused update per model)" % self._NAME)
        self.t = steps.pop() if steps else 0


def _torch_defaults(cls, **kw):
    """The ``defaults`` the installed ``torch.optim`` class makes of these arguments (its own argument checks and messages, and
    every key its ``state_dict()`` saves in a param group), taken from an instance over one scalar parameter."""
    return dict(cls([torch.zeros((), requires_grad=True)], **kw).defaults)


class FlatAdamW(FlatAdam):
    """``torch.optim.AdamW`` on the flat buffers (``mopa_adamw_flat`` / ``mopa_adamw_flat_guarded``): ``p *= 1 - lr * weight_decay``,
    then Adam's update with no L2 term in the gradient.  The state -- and with it ``state_dict()`` / ``load_state_dict()`` and the
    step count's behaviour on a skipped step -- is ``FlatAdam``'s; the param group carries what the installed ``torch.optim.AdamW``
    saves."""
    _NAME = "FlatAdamW"
    _KERNEL = "mopa_adamw_flat"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, checkpoint_shapes=None,
                 max_grad_norm=None, skip_nonfinite=False):
        super().__init__(params, lr, betas, eps, weight_decay, checkpoint_shapes, max_grad_norm, skip_nonfinite)

    @staticmethod
    def _defaults(lr, betas, eps, weight_decay):
        return _torch_defaults(torch.optim.AdamW, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)


class FlatSGD(FlatOptimizer):
    """``torch.optim.SGD`` on the flat buffers (``mopa_sgd_flat`` / ``mopa_sgd_flat_guarded``), element for element:
    ``g' = grad_scale g + wd p``; ``buf = g'`` on the first applied step (no dampening: torch clones the gradient), afterwards
    ``buf = momentum buf + (1 - dampening) g'``; ``p -= lr (g' + momentum buf | buf | g')`` (nesterov | momentum | neither).
    The param-group keys are those of the installed ``torch.optim.SGD``, its argument errors too (Nesterov needs a momentum and
    zero dampening).  ``momentum_buf`` is one flat buffer beside ``flat`` (``None`` while ``momentum == 0``).

    Which step is the first: without the guard the host knows (``_first``).  With ``skip_nonfinite`` it cannot -- whether step 1
    was applied is decided on the device -- so the guarded kernel reads one int32 of device memory, ``_valid`` (0 until a step has
    been applied; set behind the update, on the same stream, when the step record says applied): a skipped first step leaves the
    next one "first".  The word is read back in ``state_dict()`` only (and once if the guard is switched off in mid-training)."""
    _NAME = "FlatSGD"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, checkpoint_shapes=None,
                 max_grad_norm=None, skip_nonfinite=False):
        defaults = _torch_defaults(torch.optim.SGD, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                   nesterov=nesterov)
        super().__init__(params, defaults, checkpoint_shapes, max_grad_norm, skip_nonfinite)
        self.momentum_buf = torch.zeros_like(self.flat) if momentum != 0 else None
        self._first = True            # host side: True / False, None = a guarded step has run since and only _valid knows
        self._valid = torch.zeros(1, dtype=torch.int32, device=self.flat.device)

    def _buf_written(self):
        if self._first is None:
            self._first = int(self._valid) == 0
        return not self._first

    def _update(self, g, grad_scale, rec):
        mom = float(g["momentum"])
        if mom != 0.0 and self.momentum_buf is None:     # momentum switched on through param_groups after construction
            self.momentum_buf = torch.zeros_like(self.flat)
        head = (ptr(self.flat), ptr(self.grad), ptr(self.momentum_buf) if mom != 0.0 else None, self.n, float(g["lr"]), mom,
                float(g["dampening"]), float(g["weight_decay"]), int(bool(g["nesterov"])))
        if rec is None:
            first = not self._buf_written()
            call("mopa_sgd_flat", *head, int(first), grad_scale, stream())
            if first and mom != 0.0:
                self._first = False
                self._valid.fill_(1)
        else:
            call("mopa_sgd_flat_guarded", *head, ptr(self._valid), grad_scale, ptr(rec), stream())
            if self._first and mom != 0.0:
                self._first = None

    # ---- checkpointing in torch.optim.SGD's layout: per-parameter `momentum_buffer`, nothing before the first applied step,
    # nothing at all without momentum
    def state_dict(self):
        state = {}
        if self.momentum_buf is not None and self.param_groups[0]["momentum"] != 0 and self._buf_written():
            for i, (off, n) in enumerate(self._slices):
                shape = self._ckpt_shapes[i] or self.params[i].shape
                state[i] = {"momentum_buffer": self.momentum_buf[off:off + n].view(shape).clone()}
        return {"state": state, "param_groups": self._state_groups()}

    def load_state_dict(self, sd):
        self._load_groups(sd)
        bufs = {int(k): st["momentum_buffer"] for k, st in sd["state"].items() if st.get("momentum_buffer") is not None}
        if self.param_groups[0]["momentum"] == 0:
            bufs = {}
        if bufs and len(bufs) != len(self.params):
            raise ValueError("FlatSGD.load_state_dict: momentum buffers for %d of %d parameters (one fused update per model)"
                             % (len(bufs), len(self.params)))
        if self.param_groups[0]["momentum"] != 0 and self.momentum_buf is None:
            self.momentum_buf = torch.zeros_like(self.flat)
        if self.momentum_buf is not None:
            self.momentum_buf.zero_()
        for i, t in bufs.items():
            off, n = self._slices[i]
            self.momentum_buf[off:off + n].copy_(t.reshape(-1))
        self._first = not bufs        # loaded buffers mean "not first"
        self._valid.fill_(0 if self._first else 1)
