"""FlatSGD and FlatAdamW on the device (csrc/optim.hip: mopa_sgd_flat, mopa_adamw_flat and their guarded forms; mopa_amd/optim.py).

1. The C ABI against the update rule in float64 on the float32-rounded inputs and scalars.  SGD: absolute bound
   K * 2^-21 * max(1, max |want|) per array after K = 4 steps -- at most 4 roundings of <= 2^-24 relative per element and step, on
   intermediates <= 2 * max, doubled for slack; the smallest formula mistake (a dropped weight decay) moves p by 1e-3, > 60 x the
   bound.  AdamW: the project's optimizer bound, rtol 1e-5 / atol 1e-6 (tests/test_gpu_losses.py::test_flat_adam_matches_torch_adam).
2. The guarded kernels are the plain ones behind the step record: bit equality, no tolerance.
3. / 4. The classes against torch.optim.SGD / AdamW (and clip_grad_norm_) on the GPU, rtol 1e-5 / atol 1e-6.
5. FlatEMA and a Net3DSeg training loop over FlatSGD."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 7.0e7
K = 4
SIZES = (3, 4, 1203)                 # tail only; one float4; 300 float4s and a tail of 3
LRS = (0.1, 0.01)
VARIANTS = ((0.0, 0.0, 0), (0.9, 0.0, 0), (0.9, 0.1, 0), (0.9, 0.0, 1))      # momentum, dampening, nesterov
WDS = (0.0, 0.01)
GS = 0.5
RTOL, ATOL = 1e-5, 1e-6              # the project's bound for an optimizer against torch's
SHAPES = ((7, 3), (130,), (5, 5, 5), (1,))

f32 = lambda x: float(np.float32(x))
f64 = lambda x: np.float64(np.float32(x))


def _lib():
    from mopa_amd import _lib
    return _lib


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


_inputs = {}


def _normals():
    """(8, 1203) float32 normals from PCG64(2024) -- drawn once, shared, never written to; size n takes the first n columns."""
    if "x" not in _inputs:
        x = np.random.Generator(np.random.PCG64(2024)).standard_normal((8, max(SIZES))).astype(np.float32)
        x.setflags(write=False)
        _inputs["x"] = x
    return _inputs["x"]


def _rows(arrays, n):
    """The host arrays as rows of one device tensor, each row 16-byte aligned with GUARD floats behind its n elements."""
    stride = (n + 4 + 3) // 4 * 4
    host = np.full((len(arrays), stride), GUARD, np.float32)
    for r, a in enumerate(arrays):
        host[r, :n] = a
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0 and (stride * 4) % 16 == 0
    return dev


def _guards_intact(dev, n):
    tail = dev[:, n:].cpu().numpy()
    return bool((tail == np.float32(GUARD)).all())


def _rec(applied, coef):
    r = np.zeros(8, np.int32)
    r.view(np.float32)[2] = coef
    r[3] = applied
    return torch.from_numpy(r).cuda()


# ================================================================================================ 1. C ABI against float64
def _sgd_oracle(p, grads, lr, mom, damp, wd, nesterov, gs):
    p, buf = p.astype(np.float64), None
    lr, mom, damp, wd, gs = f64(lr), f64(mom), f64(damp), f64(wd), f64(gs)
    for t, g in enumerate(grads):
        gp = gs * g.astype(np.float64) + wd * p
        u = gp
        if mom != 0:
            buf = gp.copy() if t == 0 else mom * buf + (1.0 - damp) * gp
            u = gp + mom * buf if nesterov else buf
        p = p - lr * u
    return p, buf


def _sgd_run(n, lr, mom, damp, wd, nesterov, gs=GS, steps=K):
    """K steps of mopa_sgd_flat (first = 1 on step 1 only) -> (p, buf | None) as host float32, and the float64 oracle's."""
    lib = _lib()
    x = _normals()[:, :n]
    dev = _rows([x[0], x[1], np.full(n, GUARD, np.float32)], n)      # p, g, buf (never read before the first step writes it)
    for t in range(steps):
        dev[1, :n] = torch.from_numpy(x[1 + t].copy()).cuda()
        lib.call("mopa_sgd_flat", lib.ptr(dev[0]), lib.ptr(dev[1]), lib.ptr(dev[2]) if mom != 0 else None, n, f32(lr), f32(mom), f32(damp),
                 f32(wd), nesterov, int(t == 0), f32(gs), lib.stream())
    torch.cuda.synchronize()
    assert _guards_intact(dev, n), "a float behind n was written"
    host = dev.cpu().numpy()
    if mom == 0:
        assert (host[2] == np.float32(GUARD)).all(), "momentum == 0 wrote the momentum buffer"
    want_p, want_buf = _sgd_oracle(x[0], [x[1 + t] for t in range(steps)], lr, mom, damp, wd, nesterov, gs)
    return host[0, :n], (host[2, :n] if mom != 0 else None), want_p, want_buf


@pytest.mark.parametrize("n", SIZES)
def test_sgd_flat_vs_fp64(n):
    worst = 0.0
    for lr in LRS:
        for mom, damp, nesterov in VARIANTS:
            for wd in WDS:
                p, buf, want_p, want_buf = _sgd_run(n, lr, mom, damp, wd, nesterov)
                for name, got, want in (("p", p, want_p), ("buf", buf, want_buf)):
                    if want is None:
                        continue
                    bound = K * 2.0 ** -21 * max(1.0, float(np.abs(want).max()))
                    err = float(np.abs(got.astype(np.float64) - want).max())
                    worst = max(worst, err / bound)
                    print(f"n {n} lr {lr} variant {(mom, damp, nesterov)} wd {wd}: {name} max |err| {err:.3e} (bound {bound:.3e})")
                    assert err <= bound, (n, lr, mom, damp, nesterov, wd, name, err, bound)
    print(f"n {n}: worst error / bound {worst:.3f}")


def test_sgd_flat_tells_a_dropped_term_apart():
    """The oracle without weight decay, and without dampening, misses the bound by a wide margin: the test can see both."""
    p, buf, _, _ = _sgd_run(1203, 0.1, 0.9, 0.1, 0.01, 0)
    x = _normals()
    grads = [x[1 + t] for t in range(K)]
    for wrong in (_sgd_oracle(x[0], grads, 0.1, 0.9, 0.1, 0.0, 0, GS), _sgd_oracle(x[0], grads, 0.1, 0.9, 0.0, 0.01, 0, GS)):
        bound = K * 2.0 ** -21 * max(1.0, float(np.abs(wrong[0]).max()))
        assert float(np.abs(p.astype(np.float64) - wrong[0]).max()) > 60 * bound


def _adamw_oracle(p, m, v, grads, lr, b1, b2, eps, wd, gs):
    p, m, v = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    lr64, b164, b264, eps64, wd64, gs64 = f64(lr), f64(b1), f64(b2), f64(eps), f64(wd), f64(gs)
    for t, g in enumerate(grads, 1):
        gg = gs64 * g.astype(np.float64)
        p = p * (1.0 - lr64 * wd64)
        m = b164 * m + (1.0 - b164) * gg
        v = b264 * v + (1.0 - b264) * gg * gg
        bc1, bc2s = f64(1 - b1 ** t), f64(math.sqrt(1 - b2 ** t))
        p = p - lr64 / bc1 * m / (np.sqrt(v) / bc2s + eps64)
    return p, m, v


def _adamw_run(name, n, lr, wd, gs, steps=3, tail=lambda: ()):
    lib = _lib()
    x = _normals()[:, :n]
    v0 = np.abs(x[2]) * np.float32(1e-2)
    dev = _rows([x[0], x[3], x[1], v0], n)                            # p, g, exp_avg, exp_avg_sq
    b1, b2, eps = 0.9, 0.999, 1e-8
    for t in range(1, steps + 1):
        dev[1, :n] = torch.from_numpy(x[2 + t].copy()).cuda()
        lib.call(name, lib.ptr(dev[0]), lib.ptr(dev[1]), lib.ptr(dev[2]), lib.ptr(dev[3]), n, f32(lr), f32(b1), f32(b2), f32(eps), f32(wd),
                 f32(1 - b1 ** t), f32(math.sqrt(1 - b2 ** t)), f32(gs), *tail(), lib.stream())
    torch.cuda.synchronize()
    assert _guards_intact(dev, n), "a float behind n was written"
    want = _adamw_oracle(x[0], x[1], v0, [x[2 + t] for t in range(1, steps + 1)], lr, b1, b2, eps, wd, gs)
    return dev, want


@pytest.mark.parametrize("n", SIZES)
def test_adamw_flat_vs_fp64(n):
    for lr in LRS:
        dev, want = _adamw_run("mopa_adamw_flat", n, lr, 0.1, GS)
        host = dev.cpu().numpy()
        for name, row, ref in zip(("p", "exp_avg", "exp_avg_sq"), (0, 2, 3), want):
            got = host[row, :n].astype(np.float64)
            print(f"n {n} lr {lr}: {name} max |err| {np.abs(got - ref).max():.3e}, max |want| {np.abs(ref).max():.3e}")
            np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=f"{name}, n {n}, lr {lr}")
        # decoupled: the L2 form of the same decay (mopa_adam_flat) is another update, further away than the bound
        l2, _ = _adamw_run("mopa_adam_flat", n, lr, 0.1, GS)
        assert not np.allclose(l2.cpu().numpy()[0, :n], want[0], rtol=RTOL, atol=ATOL)


# ================================================================================================ 2. bits of the guarded kernels
def _sgd_once(n, mom, damp, nesterov, gs, first, rec=None, valid=None):
    """One launch on fresh buffers -> int32 bits of the (p, g, buf) rows; `rec` / `valid` given = the guarded entry point."""
    lib = _lib()
    x = _normals()[:, :n]
    dev = _rows([x[0], x[1], x[2]], n)
    head = (lib.ptr(dev[0]), lib.ptr(dev[1]), lib.ptr(dev[2]) if mom != 0 else None, n, f32(0.1), f32(mom), f32(damp), f32(0.01), nesterov)
    if rec is None:
        lib.call("mopa_sgd_flat", *head, first, f32(gs), lib.stream())
    else:
        lib.call("mopa_sgd_flat_guarded", *head, lib.ptr(valid) if valid is not None else None, f32(gs), lib.ptr(rec), lib.stream())
    torch.cuda.synchronize()
    return _bits(dev)


@pytest.mark.parametrize("n", SIZES)
def test_sgd_flat_guarded_is_sgd_flat_behind_the_record(n):
    x = _normals()[:, :n]
    init = _bits(_rows([x[0], x[1], x[2]], n))
    for mom, damp, nesterov in VARIANTS:
        for first in (1, 0):
            word = lambda: torch.tensor([0 if first else 1], dtype=torch.int32, device="cuda") if mom != 0 else None
            plain = _sgd_once(n, mom, damp, nesterov, GS, first)
            assert not torch.equal(plain[0], init[0]) and torch.equal(plain[1], init[1]) and torch.equal(plain[:, n:], init[:, n:])
            assert torch.equal(plain, _sgd_once(n, mom, damp, nesterov, GS, first)), "two runs differ"
            valid, rec = word(), _rec(1, 1.0)
            got = _sgd_once(n, mom, damp, nesterov, GS, first, rec, valid)
            assert torch.equal(got, plain), ("coef 1", mom, damp, nesterov, first)
            assert torch.equal(got, _sgd_once(n, mom, damp, nesterov, GS, first, _rec(1, 1.0), word())), "two guarded runs differ"
            assert torch.equal(rec.cpu(), _rec(1, 1.0).cpu()), "the step record was written"
            if valid is not None:
                assert int(valid) == 1, "an applied step marks the momentum buffer valid"
            valid = word()
            got = _sgd_once(n, mom, damp, nesterov, GS, first, _rec(0, 1.0), valid)
            assert torch.equal(got, init), "applied == 0 wrote"
            if valid is not None:
                assert int(valid) == (0 if first else 1), "a skipped step moved the valid word"
            half = _sgd_once(n, mom, damp, nesterov, GS, first, _rec(1, 0.5), word())
            assert torch.equal(half, _sgd_once(n, mom, damp, nesterov, f32(np.float32(GS) * np.float32(0.5)), first)), "coef 0.5"
            assert not torch.equal(half, plain)


@pytest.mark.parametrize("n", SIZES)
def test_adamw_flat_guarded_is_adamw_flat_behind_the_record(n):
    x = _normals()[:, :n]
    init = _bits(_rows([x[0], x[3], x[1], np.abs(x[2]) * np.float32(1e-2)], n))
    one = lambda name, gs, *tail: _bits(_adamw_run(name, n, 0.01, 0.1, gs, steps=1, tail=lambda: tail)[0])
    plain = one("mopa_adamw_flat", GS)
    assert torch.equal(plain, one("mopa_adamw_flat", GS)), "two runs differ"
    assert not torch.equal(plain[0], init[0]) and torch.equal(plain[1], init[1])
    rec = _rec(1, 1.0)
    assert torch.equal(one("mopa_adamw_flat_guarded", GS, rec.data_ptr()), plain), "coef 1"
    assert torch.equal(one("mopa_adamw_flat_guarded", GS, rec.data_ptr()), plain), "two guarded runs differ"
    assert torch.equal(rec.cpu(), _rec(1, 1.0).cpu())
    skip = _rec(0, 1.0)
    assert torch.equal(one("mopa_adamw_flat_guarded", GS, skip.data_ptr()), init), "applied == 0 wrote (the decay is part of the step)"
    half = _rec(1, 0.5)
    assert torch.equal(one("mopa_adamw_flat_guarded", GS, half.data_ptr()), one("mopa_adamw_flat", f32(np.float32(GS) * np.float32(0.5))))


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib()
    buf = torch.full((4, 16), 1.0, device="cuda")
    rec, valid = _rec(1, 1.0), torch.zeros(4, dtype=torch.int32, device="cuda")
    ptrs = [lib.ptr(buf[i]) for i in range(4)]
    r, w = lib.ptr(rec), lib.ptr(valid)
    adam = (1e-2, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.1, 1.0)

    def refused(name, *args):
        with pytest.raises(RuntimeError, match="code -1"):
            lib.call(name, *args, lib.stream())

    for bad, n in ((ptrs, 0), (ptrs, -4), ([ptrs[0] + 4] + ptrs[1:], 8), ([ptrs[0], ptrs[1] + 4] + ptrs[2:], 8),
                   (ptrs[:2] + [ptrs[2] + 4, ptrs[3]], 8), (ptrs[:3] + [ptrs[3] + 4], 8)):
        refused("mopa_adamw_flat", *bad, n, *adam)
        refused("mopa_adamw_flat_guarded", *bad, n, *adam, r)
    refused("mopa_adamw_flat_guarded", *ptrs, 8, *adam, r + 4)
    refused("mopa_adamw_flat_guarded", *ptrs, 8, *adam, None)
    sgd = (0.1, 0.9, 0.1, 0.01, 0)
    for bad, n in ((ptrs[:3], 0), (ptrs[:3], -4), ([ptrs[0] + 4] + ptrs[1:3], 8), ([ptrs[0], ptrs[1] + 4, ptrs[2]], 8),
                   (ptrs[:2] + [ptrs[2] + 4], 8), (ptrs[:2] + [None], 8)):       # (momentum != 0 needs its buffer)
        refused("mopa_sgd_flat", *bad, n, *sgd, 1, 1.0)
        refused("mopa_sgd_flat_guarded", *bad, n, *sgd, w, 1.0, r)
    refused("mopa_sgd_flat_guarded", *ptrs[:3], 8, *sgd, w, 1.0, r + 4)
    refused("mopa_sgd_flat_guarded", *ptrs[:3], 8, *sgd, w, 1.0, None)
    refused("mopa_sgd_flat_guarded", *ptrs[:3], 8, *sgd, w + 2, 1.0, r)
    refused("mopa_sgd_flat_guarded", *ptrs[:3], 8, *sgd, None, 1.0, r)
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all()) and torch.equal(rec.cpu(), _rec(1, 1.0).cpu()) and not bool(valid.any())
    # ... and with nothing wrong the calls go through; momentum == 0 takes neither a buffer nor a valid word
    lib.call("mopa_sgd_flat_guarded", ptrs[0], ptrs[1], None, 8, 0.1, 0.0, 0.0, 0.0, 0, None, 1.0, r, lib.stream())
    lib.call("mopa_sgd_flat", ptrs[2], ptrs[1], None, 8, 0.1, 0.0, 0.0, 0.0, 0, 1, 1.0, lib.stream())
    want = float(np.float32(1.0) - np.float32(0.1))
    assert buf[0, :8].tolist() == [pytest.approx(want, abs=1e-7)] * 8 and torch.equal(buf[0, :8], buf[2, :8])
    assert bool((buf[0, 8:] == 1.0).all()) and bool((buf[1] == 1.0).all()) and bool((buf[3] == 1.0).all())


# ================================================================================================ 3. the classes against torch
def _pair(seed=0):
    torch.manual_seed(seed)
    ps = [torch.randn(s, device="cuda").requires_grad_(True) for s in SHAPES]
    return ps, [p.detach().clone().requires_grad_(True) for p in ps]


def _sin_steps(ps, qs, opt, ref, steps=5, before_ref_step=None):
    for it in range(steps):
        opt.zero_grad()
        ref.zero_grad()
        for p, q in zip(ps, qs):
            (p.sin() * (it + 1)).sum().backward()
            (q.sin() * (it + 1)).sum().backward()
        if before_ref_step is not None:
            before_ref_step()
        opt.step()
        ref.step()


def _assert_close(ps, qs, what):
    for i, (p, q) in enumerate(zip(ps, qs)):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=f"{what}, parameter {i}")


@pytest.mark.parametrize("mom,damp,nesterov", VARIANTS)
@pytest.mark.parametrize("wd", WDS)
def test_flat_sgd_matches_torch_sgd(wd, mom, damp, nesterov):
    from mopa_amd.optim import FlatSGD
    ps, qs = _pair()
    kw = dict(lr=1e-2, momentum=mom, dampening=damp, weight_decay=wd, nesterov=bool(nesterov))
    opt, ref = FlatSGD(ps, **kw), torch.optim.SGD(qs, **kw)
    start = [p.detach().clone() for p in ps]
    _sin_steps(ps, qs, opt, ref)
    _assert_close(ps, qs, "FlatSGD vs torch.optim.SGD")
    assert all(not torch.equal(p.detach(), s) for p, s in zip(ps, start))
    sd, rd = opt.state_dict()["state"], ref.state_dict()["state"]
    if mom == 0:
        assert sd == {}
    else:
        for i in range(len(ps)):
            np.testing.assert_allclose(sd[i]["momentum_buffer"].cpu().numpy(), rd[i]["momentum_buffer"].cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_flat_adamw_matches_torch_adamw():
    from mopa_amd.optim import FlatAdam, FlatAdamW
    ps, qs = _pair()
    opt, ref = FlatAdamW(ps, lr=1e-2, weight_decay=0.1), torch.optim.AdamW(qs, lr=1e-2, weight_decay=0.1)
    _sin_steps(ps, qs, opt, ref)
    _assert_close(ps, qs, "FlatAdamW vs torch.optim.AdamW")
    sd, rd = opt.state_dict()["state"], ref.state_dict()["state"]
    for i in range(len(ps)):
        assert float(sd[i]["step"]) == float(rd[i]["step"]) == 5.0
        for k in ("exp_avg", "exp_avg_sq"):
            np.testing.assert_allclose(sd[i][k].cpu().numpy(), rd[i][k].cpu().numpy(), rtol=RTOL, atol=ATOL)
    # FlatAdam at the same weight decay (L2) is another optimizer, and this comparison sees it
    ls, ms = _pair()
    l2, l2_ref = FlatAdam(ls, lr=1e-2, weight_decay=0.1), torch.optim.Adam(ms, lr=1e-2, weight_decay=0.1)
    _sin_steps(ls, ms, l2, l2_ref)
    _assert_close(ls, ms, "FlatAdam vs torch.optim.Adam")
    a = np.concatenate([p.detach().cpu().numpy().ravel() for p in ps])
    b = np.concatenate([p.detach().cpu().numpy().ravel() for p in ls])
    assert not np.allclose(a, b, rtol=RTOL, atol=ATOL)
    assert float(np.max(np.abs(a - b) - (ATOL + RTOL * np.abs(b)))) > 0


# ================================================================================================ 4. the guard
def test_flat_sgd_clipping_matches_clip_grad_norm():
    from mopa_amd.optim import FlatSGD
    M = 5.0                          # the sin losses' gradient norm is ~12 * (it + 1): every step clips
    ps, qs = _pair()
    kw = dict(lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=0.01)
    opt, ref = FlatSGD(ps, max_grad_norm=M, **kw), torch.optim.SGD(qs, **kw)
    seen = []

    def clip():
        seen.append([_bits(p.grad).clone() for p in ps])
        torch.nn.utils.clip_grad_norm_(qs, M)

    _sin_steps(ps, qs, opt, ref, before_ref_step=clip)
    _assert_close(ps, qs, "FlatSGD(max_grad_norm) vs clip_grad_norm_ + torch.optim.SGD")
    assert int(opt.last_stats.n_clipped) == 5 and int(opt.last_stats.n_skipped) == 0 and float(opt.last_stats.coef) < 1.0
    for p, b in zip(ps, seen[-1]):
        assert torch.equal(_bits(p.grad), b), "clipping rewrote .grad"
    loose_p, loose_q = _pair()       # ... and without the guard the result is another one
    _sin_steps(loose_p, loose_q, FlatSGD(loose_p, **kw), torch.optim.SGD(loose_q, **kw))
    assert not np.allclose(loose_p[1].detach().cpu().numpy(), ps[1].detach().cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_a_skipped_first_step_leaves_the_next_one_first():
    from mopa_amd.optim import FlatSGD
    rng = np.random.Generator(np.random.PCG64(31))
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda()) for s in SHAPES]
    lr, mom, damp, wd = 0.1, 0.9, 0.1, 0.01
    opt = FlatSGD(ps, lr=lr, momentum=mom, dampening=damp, weight_decay=wd, skip_nonfinite=True)
    opt.momentum_buf.fill_(3.0)      # whatever is in the buffer before the first applied step must not reach it
    g1 = [torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda() for s in SHAPES]
    g2 = [torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda() for s in SHAPES]
    g1[2].view(-1)[17] = float("nan")
    for p, g in zip(ps, g1):
        p.grad.copy_(g)
    before = [_bits(opt.flat).clone(), _bits(opt.momentum_buf).clone()]
    p0 = opt.flat.detach().cpu().numpy().astype(np.float64)
    opt.step()
    st = opt.last_stats
    assert int(st.applied) == 0 and int(st.n_skipped) == 1 and int(st.nonfinite) == 1
    assert torch.equal(_bits(opt.flat), before[0]) and torch.equal(_bits(opt.momentum_buf), before[1]), "a skipped step wrote"
    assert opt.state_dict()["state"] == {}
    for p, g in zip(ps, g2):
        p.grad.copy_(g)
    opt.step()
    assert int(opt.last_stats.applied) == 1 and int(opt.last_stats.n_skipped) == 1
    gp = opt.grad.detach().cpu().numpy().astype(np.float64) + f64(wd) * p0          # g' of step 2
    bound = 2.0 ** -21 * max(1.0, float(np.abs(gp).max()))                          # the bound of (1), one step
    live = np.zeros(opt.n, bool)
    for off, n in opt._slices:
        live[off:off + n] = True
    buf = opt.momentum_buf.detach().cpu().numpy().astype(np.float64)
    err_first, err_later = np.abs(buf - gp)[live].max(), np.abs(buf - (f64(mom) * 3.0 + (1 - f64(damp)) * gp))[live].max()
    print(f"momentum buffer after the first applied step: max |buf - g'| {err_first:.3e} (bound {bound:.3e}); as a later step {err_later:.3e}")
    assert err_first <= bound and err_later > 100 * bound
    assert np.abs(buf - 0.9 * gp)[live].max() > 100 * bound
    assert np.abs(opt.flat.detach().cpu().numpy() - (p0 - f64(lr) * gp))[live].max() <= bound
    sd = opt.state_dict()["state"]
    assert sorted(sd) == list(range(len(SHAPES))) and torch.equal(sd[1]["momentum_buffer"], opt.momentum_buf[opt._slices[1][0]:][:130])
    for p, g in zip(ps, g2):         # a third step is not the first: buf = momentum buf + (1 - dampening) g'
        p.grad.copy_(g)
    p1 = opt.flat.detach().cpu().numpy().astype(np.float64)
    opt.step()
    want = f64(mom) * buf + (1 - f64(damp)) * (opt.grad.detach().cpu().numpy().astype(np.float64) + f64(wd) * p1)
    assert np.abs(opt.momentum_buf.detach().cpu().numpy() - want)[live].max() <= 2 * bound


def test_guard_that_does_not_trigger_is_the_plain_optimizer():
    from mopa_amd.optim import FlatAdamW, FlatSGD
    for make in (lambda ps, **kw: FlatSGD(ps, lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=0.01, **kw),
                 lambda ps, **kw: FlatAdamW(ps, lr=1e-2, weight_decay=0.1, **kw)):
        ps, qs = _pair()
        plain, guarded = make(ps), make(qs, max_grad_norm=1e9, skip_nonfinite=True)
        _sin_steps(ps, qs, plain, guarded)
        assert torch.equal(_bits(plain.flat), _bits(guarded.flat)) and int(guarded.last_stats.n_clipped) == 0
        a, b = plain.state_dict()["state"], guarded.state_dict()["state"]
        assert sorted(a) == sorted(b) == list(range(len(SHAPES)))
        for i in a:
            for k in a[i]:
                assert torch.equal(a[i][k], b[i][k]), (i, k)


# ================================================================================================ 5. around the optimizer
def test_flat_ema_over_flat_sgd():
    from mopa_amd.optim import FlatSGD
    from mopa_amd.pseudo import FlatEMA
    ps, qs = _pair()
    opt = FlatSGD(ps, lr=1e-2, momentum=0.9)
    ema = FlatEMA(opt, 0.99)
    start = opt.flat.detach().cpu().numpy().astype(np.float64)
    _sin_steps(ps, qs, opt, torch.optim.SGD(qs, lr=1e-2, momentum=0.9), steps=1)
    ema.update()
    live = opt.flat.detach().cpu().numpy().astype(np.float64)
    decay = min(0.99, 2.0 / 11.0)
    want = f64(decay) * start + (1.0 - f64(decay)) * live
    # shadow -= (1 - decay) * (shadow - param): three roundings (1 - decay, the difference, the product) on a term <= 2 max, one on
    # the result <= max: 7 * 2^-24 * max, rounded up to 8
    bound = 8 * 2.0 ** -24 * max(1.0, float(np.abs(start).max()), float(np.abs(live).max()))
    assert np.abs(ema.shadow.cpu().numpy() - want).max() <= bound and not np.array_equal(start, live)
    saved = [_bits(p).clone() for p in ps]
    with ema.average_parameters():
        for p, (off, n) in zip(ps, opt._slices):
            assert torch.equal(p.detach().reshape(-1), ema.shadow[off:off + n])
    for p, b in zip(ps, saved):
        assert torch.equal(_bits(p), b), "average_parameters did not restore the weights"


def test_net3dseg_trains_with_flat_sgd():
    from mopa_amd.common.solver.build import build_optimizer
    from mopa_amd.config import Node, default_cfg
    from mopa_amd.models.build import build_model_3d
    from mopa_amd.models.scn_unet import checkpoint_shapes
    from mopa_amd.optim import FlatSGD
    torch.manual_seed(0)
    cfg = default_cfg()
    cfg.MODEL_3D.SCN.num_planes = 4
    model, _ = build_model_3d(cfg)
    model = model.cuda().train()
    rng = np.random.Generator(np.random.PCG64(5))
    n = 2000
    centers = rng.integers(4, 44, (40, 3))
    xyz = np.clip(centers[rng.integers(0, 40, n)] + rng.integers(-3, 4, (n, 3)), 0, 47)
    coords = torch.from_numpy(np.concatenate([xyz, rng.integers(0, 2, (n, 1))], 1).astype(np.int64))
    feats = torch.from_numpy(rng.random((n, 1), dtype=np.float32) + 0.5).cuda()
    opt = build_optimizer(Node(TYPE="SGD", BASE_LR=0.05, WEIGHT_DECAY=1e-4, SGD=Node(momentum=0.9, dampening=0.0)), model, model_type="3D",
                          max_grad_norm=10.0, skip_nonfinite=True)
    assert type(opt) is FlatSGD and opt._ckpt_shapes == checkpoint_shapes(model)
    start = opt.flat.clone()
    logits = []
    for _ in range(2):
        opt.zero_grad()
        out = model({"x": [coords, feats]})
        logits.append(out["seg_logit"].detach().clone())
        sum(v.square().mean() for v in out.values() if torch.is_tensor(v) and v.is_floating_point() and v.requires_grad).backward()
        opt.step()
        assert int(opt.last_stats.applied) == 1
    assert bool(torch.isfinite(opt.flat).all()) and not torch.equal(opt.flat, start)
    assert logits[0].shape == logits[1].shape and not torch.equal(logits[0], logits[1]), "the second forward ran on stale weight forms"
    sd = opt.state_dict()["state"]
    assert len(sd) == len(opt.params)
    assert [tuple(sd[i]["momentum_buffer"].shape) for i in sd] == [tuple(s or p.shape) for s, p in zip(opt._ckpt_shapes, opt.params)]
