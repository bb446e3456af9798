"""FlatAdam's gradient guard on the device (csrc/optim.hip: mopa_grad_stats, mopa_adam_flat_guarded; mopa_amd/optim.py).

Statistics against numpy float64 at rtol 2^-23, atol 0: a float product is exact in double, a double sum of fewer than 2^25 terms
errs below 2^-28 relative, the double square root adds 2^-53, and ONE rounding to float (2^-24) remains.  Everything about the
update itself is bit equality with mopa_adam_flat -- the two kernels share one body -- so no second tolerance appears anywhere."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 2.0 ** -23
GUARD = 7.0e7
SCALES = (1.0, 0.5, -0.25)


def _lib():
    from mopa_amd import _lib
    return _lib


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _lengths(chunk):
    return [1, 2, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 65 * chunk + 3] + [1 + i % 7 for i in range(300)]


_case = {}


def _stats_case():
    """The parameter list of the statistics tests, its gradients (magnitudes 1e-20 .. 1e+15 across parameters) and the float64
    reference -- built once, shared, never written to."""
    if _case:
        return _case
    lib = _lib()
    chunk = lib.query("mopa_grad_stats_chunk")
    lengths = _lengths(chunk)
    slices, off = [], 0
    for n in lengths:
        slices.append((off, n))
        off += (n + 3) // 4 * 4
    rng = np.random.Generator(np.random.PCG64(18))
    expo = rng.permutation(np.linspace(-20.0, 15.0, len(lengths)))
    flat = np.full(off, np.nan, np.float32)      # NaN in the padding: no chunk may read it
    for (o, n), e in zip(slices, expo):
        flat[o:o + n] = (rng.standard_normal(n) * 10.0 ** e).astype(np.float32)
    assert off < 1_000_000
    sumsq = np.array([np.sum(flat[o:o + n].astype(np.float64) ** 2) for o, n in slices])
    _case.update(chunk=chunk, lengths=lengths, slices=slices, n=off, flat=flat, sumsq=sumsq,
                 absmax=np.array([np.abs(flat[o:o + n].astype(np.float64)).max() for o, n in slices]))
    for v in _case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return _case


def _run_stats(flat_np, slices, grad_scale, max_norm=0.0, skip=0, rec0=None):
    """mopa_grad_stats through the C ABI on buffers of this test's own, each with guard floats behind it.
    -> dict of host arrays; asserts the guards."""
    from mopa_amd.optim import stat_chunks
    lib = _lib()
    P = len(slices)
    tab = torch.tensor(stat_chunks(slices, lib.query("mopa_grad_stats_chunk")), dtype=torch.int64).cuda()
    n_chunks = tab.shape[0]
    ws_bytes = lib.query("mopa_grad_stats_workspace_bytes", n_chunks)
    assert ws_bytes % 4 == 0
    g = torch.tensor(flat_np).cuda()
    stats = torch.full((3 * P + 4,), GUARD, device="cuda")
    rec = torch.full((8 + 4,), GUARD, device="cuda")
    rec[:8].view(torch.int32).copy_(torch.zeros(8, dtype=torch.int32) if rec0 is None else torch.from_numpy(rec0))
    ws = torch.full((ws_bytes // 4 + 4,), GUARD, device="cuda")
    lib.call("mopa_grad_stats", lib.ptr(g), lib.ptr(tab), n_chunks, P, grad_scale, max_norm, skip, lib.ptr(stats), lib.ptr(rec), lib.ptr(ws),
             ws_bytes, lib.stream())
    torch.cuda.synchronize()
    guard_bits = _bits(torch.full((4,), GUARD))
    assert torch.equal(_bits(stats[3 * P:]), guard_bits), "a float behind stats was written"
    assert torch.equal(_bits(rec[8:]), guard_bits), "a float behind rec was written"
    assert torch.equal(_bits(ws[ws_bytes // 4:]), guard_bits), "a float behind the workspace was written"
    assert torch.equal(_bits(g), _bits(torch.tensor(flat_np))), "the gradient was written"
    s, r = stats[:3 * P].cpu(), rec[:8].cpu()
    ri = r.view(torch.int32).numpy()
    return dict(param_norm=s[:P].numpy(), param_absmax=s[P:2 * P].numpy(), param_nonfinite=s[2 * P:].view(torch.int32).numpy(),
                norm=r.numpy()[0], nonfinite=int(ri[1]), coef=r.numpy()[2], applied=int(ri[3]),
                n_skipped=int(r[4:8].view(torch.int64)[0]), n_clipped=int(r[4:8].view(torch.int64)[1]), rec=ri.copy())


# ------------------------------------------------------------------------------------------------ 1. statistics against fp64
@pytest.mark.parametrize("grad_scale", SCALES)
def test_grad_stats_vs_fp64(grad_scale):
    c = _stats_case()
    got = _run_stats(c["flat"], c["slices"], grad_scale)
    ref_pn = np.sqrt(c["sumsq"]) * abs(grad_scale)
    ref_n = math.sqrt(c["sumsq"].sum()) * abs(grad_scale)
    ref_am = c["absmax"] * abs(grad_scale)
    rel = lambda a, b: float(np.max(np.abs(a.astype(np.float64) - b) / np.abs(b)))
    print(f"grad_scale {grad_scale}: worst relative error param_norm {rel(got['param_norm'], ref_pn):.3e}, "
          f"norm {abs(float(got['norm']) - ref_n) / ref_n:.3e}, param_absmax {rel(got['param_absmax'], ref_am):.3e} (bound {RTOL:.3e})")
    np.testing.assert_allclose(got["param_norm"].astype(np.float64), ref_pn, rtol=RTOL, atol=0)
    np.testing.assert_allclose(float(got["norm"]), ref_n, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got["param_absmax"].astype(np.float64), ref_am, rtol=RTOL, atol=0)
    assert not got["param_nonfinite"].any() and got["nonfinite"] == 0
    assert got["coef"] == 1.0 and got["applied"] == 1 and got["n_skipped"] == 0 and got["n_clipped"] == 0
    again = _run_stats(c["flat"], c["slices"], grad_scale)
    for k in ("param_norm", "param_absmax", "param_nonfinite", "rec"):
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), k


# ------------------------------------------------------------------------------------------------ 2. non-finite accounting
def test_grad_stats_counts_non_finite_elements():
    c = _stats_case()
    chunk, slices = c["chunk"], c["slices"]
    clean = _run_stats(c["flat"], slices, 1.0)
    flat = c["flat"].copy()
    assert c["lengths"][4] == 5 and c["lengths"][8] == 2 * chunk + 5 and c["lengths"][9] == 65 * chunk + 3
    flat[slices[4][0] + 4] = np.nan                  # the last element of a 5-float parameter (the scalar tail)
    flat[slices[8][0]] = np.inf                      # element 0 of a multi-chunk parameter
    flat[slices[9][0] + chunk - 1] = -np.inf         # the last element of a chunk
    got = _run_stats(flat, slices, 1.0)
    want = np.zeros(len(slices), np.int32)
    want[[4, 8, 9]] = 1
    assert np.array_equal(got["param_nonfinite"], want) and got["nonfinite"] == 3
    others = np.ones(len(slices), bool)
    others[[4, 8, 9]] = False
    assert np.array_equal(got["param_norm"].view(np.int32)[others], clean["param_norm"].view(np.int32)[others])
    assert np.array_equal(got["param_absmax"].view(np.int32)[others], clean["param_absmax"].view(np.int32)[others])
    assert np.isnan(got["param_norm"][4]) and got["param_norm"][8] == np.inf and got["param_norm"][9] == np.inf
    for i in (4, 8, 9):                              # max |g| is over the finite elements
        o, n = slices[i]
        fin = flat[o:o + n][np.isfinite(flat[o:o + n])]
        assert got["param_absmax"][i] == np.abs(fin).max()
    assert np.isnan(got["norm"])
    assert got["applied"] == 1 and got["n_skipped"] == 0          # nobody asked to skip
    flat[slices[4][0] + 4] = c["flat"][slices[4][0] + 4]
    got = _run_stats(flat, slices, 1.0, skip=1, rec0=np.array([0, 0, 0, 0, 5, 0, 7, 0], np.int32))
    assert got["norm"] == np.inf and got["nonfinite"] == 2
    assert got["applied"] == 0 and got["n_skipped"] == 6 and got["n_clipped"] == 7   # the counters are running ones


# ------------------------------------------------------------------------------------------------ optimizers over ~70 k floats
SHAPES = ((64, 1000), (5,), (3, 7, 11), (4099,), (1,))


def _opt(seed=3, **kw):
    from mopa_amd.optim import FlatAdam
    rng = np.random.Generator(np.random.PCG64(seed))
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda()) for s in SHAPES]
    return FlatAdam(params, lr=1e-2, **kw)


def _grads(seed):
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    return [torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda() for s in SHAPES]


def _set_grads(opt, grads):
    for p, g in zip(opt.params, grads):
        p.grad.copy_(g)


def _same_state(a, b):
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name


# ------------------------------------------------------------------------------------------------ 3. nothing triggers
@pytest.mark.parametrize("grad_scale", (1.0, 0.5))
@pytest.mark.parametrize("weight_decay", (0.0, 0.01))
def test_guard_that_does_not_trigger_is_the_plain_optimizer(weight_decay, grad_scale):
    plain = _opt(weight_decay=weight_decay)
    guarded = _opt(weight_decay=weight_decay, skip_nonfinite=True, max_grad_norm=1e9)
    assert guarded.n > 68_000
    for t in range(5):
        g = _grads(t)
        _set_grads(plain, g)
        _set_grads(guarded, g)
        plain.step(grad_scale)
        guarded.step(grad_scale)
        _same_state(plain, guarded)
        st = guarded.last_stats
        assert float(st.coef) == 1.0 and int(st.applied) == 1 and int(st.n_skipped) == 0 and int(st.n_clipped) == 0
        assert int(st.nonfinite) == 0
    assert not torch.equal(plain.flat, _opt().flat) and plain.last_stats is None


# ------------------------------------------------------------------------------------------------ 4. clipping
@pytest.mark.parametrize("grad_scale", (1.0, 0.5))
def test_clipping_is_the_plain_step_with_the_scaled_gradient(grad_scale):
    g = _grads(7)
    probe = _opt()
    _set_grads(probe, g)
    norm = float(probe.grad_stats(grad_scale).norm)
    ref = abs(grad_scale) * math.sqrt(sum(float(x.double().square().sum()) for x in g))
    np.testing.assert_allclose(norm, ref, rtol=RTOL, atol=0)
    max_norm = norm / 10.0
    guarded = _opt(weight_decay=0.01, max_grad_norm=max_norm)
    plain = _opt(weight_decay=0.01)
    _set_grads(guarded, g)
    _set_grads(plain, g)
    before = _bits(guarded.grad).clone()
    guarded.step(grad_scale)
    st = guarded.last_stats
    coef = np.float32(max_norm) / (np.float32(float(st.norm)) + np.float32(1e-6))   # clip_grad_norm_'s formula in float32
    assert isinstance(coef, np.float32) and coef < 1.0
    assert np.float32(float(st.coef)) == coef
    plain.step(float(np.float32(grad_scale) * coef))
    _same_state(plain, guarded)
    assert int(st.n_clipped) == 1 and int(st.n_skipped) == 0 and int(st.applied) == 1
    assert torch.equal(_bits(guarded.grad), before), "clipping rewrote the gradient"
    for p, x in zip(guarded.params, g):
        assert torch.equal(p.grad, x)


# ------------------------------------------------------------------------------------------------ 5. skip
def test_non_finite_gradient_skips_the_step():
    from mopa_amd.pseudo import FlatEMA
    guarded, plain, loose = _opt(skip_nonfinite=True), _opt(), _opt()
    ema = FlatEMA(guarded, decay=0.9)
    g0, g1 = _grads(20), _grads(21)
    for o in (guarded, plain, loose):
        _set_grads(o, g0)
        o.step()
    ema.update()
    _same_state(plain, guarded)
    bad = [x.clone() for x in g1]
    bad[2].view(-1)[17] = float("nan")
    _set_grads(guarded, bad)
    before = [_bits(t).clone() for t in (guarded.flat, guarded.exp_avg, guarded.exp_avg_sq)]
    guarded.step()
    ema.update()
    st = guarded.last_stats
    assert int(st.applied) == 0 and int(st.n_skipped) == 1 and int(st.nonfinite) == 1 and int(st.n_clipped) == 0
    assert int(st.param_nonfinite[2]) == 1 and int(st.param_nonfinite.sum()) == 1
    for t, b in zip((guarded.flat, guarded.exp_avg, guarded.exp_avg_sq), before):
        assert torch.equal(_bits(t), b), "a skipped step wrote"
    assert guarded.t == 2
    _set_grads(guarded, g1)
    guarded.step()
    ema.update()
    assert int(guarded.last_stats.applied) == 1 and int(guarded.last_stats.n_skipped) == 1
    plain.t += 1                     # the documented deviation: t advances on a skipped step
    _set_grads(plain, g1)
    plain.step()
    _same_state(plain, guarded)
    assert bool(torch.isfinite(ema.shadow).all()) and bool(torch.isfinite(guarded.flat).all())
    _set_grads(loose, bad)           # the same NaN without the guard: it is the guard that made the difference
    loose.step()
    assert bool(torch.isnan(loose.flat).any())


# ------------------------------------------------------------------------------------------------ 6. through the C ABI
def _rec(applied, coef):
    r = np.zeros(8, np.int32)
    r.view(np.float32)[2] = coef
    r[3] = applied
    return torch.from_numpy(r).cuda()


@pytest.mark.parametrize("n", (1, 3, 5, 1203))
def test_adam_flat_guarded_is_adam_flat_behind_the_record(n):
    lib = _lib()
    rng = np.random.Generator(np.random.PCG64(n))
    stride = (n + 4 + 3) // 4 * 4
    init = np.full((4, stride), GUARD, np.float32)
    init[:, :n] = rng.standard_normal((4, n), dtype=np.float32)
    init[3, :n] = np.abs(init[3, :n])                  # exp_avg_sq >= 0
    f32 = lambda x: float(np.float32(x))
    lr, b1, b2, eps, wd, gs = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.01), f32(0.5)
    bc1, bc2s = f32(1 - 0.9 ** 3), f32(math.sqrt(1 - 0.999 ** 3))

    def run(name, scale, *tail):
        buf = torch.from_numpy(init.copy()).cuda()
        assert buf.data_ptr() % 16 == 0
        lib.call(name, lib.ptr(buf[0]), lib.ptr(buf[1]), lib.ptr(buf[2]), lib.ptr(buf[3]), n, lr, b1, b2, eps, wd, bc1, bc2s, scale,
                 *tail, lib.stream())
        return _bits(buf)

    for coef in (1.0, 0.5):
        rec = _rec(1, coef)
        want = run("mopa_adam_flat", f32(np.float32(gs) * np.float32(coef)))
        got = run("mopa_adam_flat_guarded", gs, lib.ptr(rec))
        assert torch.equal(got, want), coef           # the floats behind n included
        assert not torch.equal(got, _bits(torch.from_numpy(init)))
        assert torch.equal(_bits(torch.from_numpy(init))[:, n:], got[:, n:]) and torch.equal(got[1], _bits(torch.from_numpy(init))[1])
        assert torch.equal(rec.cpu(), _rec(1, coef).cpu())
        assert torch.equal(run("mopa_adam_flat_guarded", gs, lib.ptr(_rec(0, coef))), _bits(torch.from_numpy(init))), "applied == 0 wrote"


def test_bad_arguments_are_refused_before_any_launch():
    from mopa_amd.optim import stat_chunks
    lib = _lib()
    buf = torch.full((4, 16), 1.0, device="cuda")
    rec = _rec(1, 1.0)
    args = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.1, 1.0)
    ptrs = [lib.ptr(buf[i]) for i in range(4)]
    for bad_ptrs, n, r in ((ptrs, 0, lib.ptr(rec)), (ptrs, -4, lib.ptr(rec)), ([ptrs[0] + 4] + ptrs[1:], 8, lib.ptr(rec)),
                           (ptrs[:3] + [ptrs[3] + 4], 8, lib.ptr(rec)), (ptrs, 8, lib.ptr(rec) + 4), (ptrs, 8, None)):
        with pytest.raises(RuntimeError, match="code -1"):
            lib.call("mopa_adam_flat_guarded", *bad_ptrs, n, *args, r, lib.stream())
    tab = torch.tensor(stat_chunks([(0, 16), (16, 16)], 8192), dtype=torch.int64).cuda()
    g = torch.ones(32, device="cuda")
    stats = torch.full((6,), GUARD, device="cuda")
    ws_bytes = lib.query("mopa_grad_stats_workspace_bytes", 2)
    ws = torch.full((ws_bytes // 4 + 4,), GUARD, device="cuda")
    ok = (lib.ptr(g), lib.ptr(tab), 2, 2, 1.0, 0.0, 0, lib.ptr(stats), lib.ptr(rec), lib.ptr(ws), ws_bytes)
    for pos, val, code in ((10, ws_bytes - 1, -2), (2, 0, -1), (3, 0, -1), (0, ok[0] + 4, -1), (9, ok[9] + 8, -1), (8, ok[8] + 4, -1),
                           (1, None, -1), (7, None, -1)):
        a = list(ok)
        a[pos] = val
        with pytest.raises(RuntimeError, match=f"code {code}"):
            lib.call("mopa_grad_stats", *a, lib.stream())
    torch.cuda.synchronize()
    assert bool((buf == 1.0).all()) and bool((stats == GUARD).all()) and bool((ws == GUARD).all())
    assert torch.equal(rec.cpu(), _rec(1, 1.0).cpu())
    lib.call("mopa_grad_stats", *ok, lib.stream())    # ... and the same call with nothing wrong goes through
    assert stats[:2].tolist() == [4.0, 4.0] and float(rec.view(torch.float32)[0]) == float(np.float32(math.sqrt(32.0)))


# ------------------------------------------------------------------------------------------------ 7. one real backward pass
def test_param_norms_of_a_real_backward_pass():
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_3d
    from mopa_amd.optim import FlatAdam
    torch.manual_seed(0)
    cfg = default_cfg()
    cfg.MODEL_3D.SCN.num_planes = 4
    model, _ = build_model_3d(cfg)
    model = model.cuda().train()
    rng = np.random.Generator(np.random.PCG64(5))
    n = 2000
    centers = rng.integers(4, 44, (40, 3))
    xyz = np.clip(centers[rng.integers(0, 40, n)] + rng.integers(-3, 4, (n, 3)), 0, 47)
    coords = np.concatenate([xyz, rng.integers(0, 2, (n, 1))], 1).astype(np.int64)
    feats = torch.from_numpy(rng.random((n, 1), dtype=np.float32) + 0.5).cuda()
    opt = FlatAdam(model.parameters(), lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    opt.zero_grad()
    out = model({"x": [torch.from_numpy(coords), feats]})
    sum(v.square().mean() for v in out.values() if torch.is_tensor(v) and v.is_floating_point() and v.requires_grad).backward()
    opt.step()
    st = opt.last_stats
    ref = torch.stack([p.grad.double().norm() for p in opt.params]).cpu().numpy()
    got = st.param_norm.cpu().numpy().astype(np.float64)
    assert ref.max() > 0 and len(ref) == len(opt.params) > 10
    print("worst relative error of param_norm: %.3e of %d parameters" % (np.max(np.abs(got - ref) / np.maximum(ref, 1e-300)), len(ref)))
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)
    np.testing.assert_allclose(float(st.norm), math.sqrt((ref ** 2).sum()), rtol=RTOL, atol=0)
    assert int(st.applied) == 1 and int(st.nonfinite) == 0
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    line = st.summary(names, top=3)
    assert names[int(np.argmax(ref))] in line and "applied" in line
