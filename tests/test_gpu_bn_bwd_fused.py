"""BatchNorm backward of the image branch without the two passes the result does not need (csrc/rows.hip, round 11):

  * mopa_bn_act_fwd_groups_bits leaves one bit per element of a residual layer, pre-activation > 0, and mopa_bn_act_bwd_groups_fused
    reads that bit instead of the saved output;
  * mopa_bn_act_bwd_groups_fused leaves mopa_colsum's partial sums of the dx it writes, mopa_colsum_reduce turns them into the bias
    gradient of the convolution in front of the BatchNorm.

Neither may change one bit: the yardstick is the existing entry points (mopa_bn_act_fwd_groups, mopa_bn_act_bwd_groups with ymask = y,
mopa_colsum on the written dx) under torch.equal.  Those entry points keep their kernels' arithmetic, but the apply kernel's row body
is now shared source (bn_bwd_apply_row), so an error in it would show on both sides: what is independent of this change is the fp64
formula below, the untouched existing suite and a bit comparison of the benchmark's outputs against the parent commit.  The fp64 formula
is checked at the tolerances tests/test_gpu_2d.py uses for the BatchNorm
backward (rtol 1e-3 / atol 1e-4 of the tensor's scale; the residual gradient rtol 1e-4 / atol 2e-5)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, MOM = 1e-5, 0.1
PAD, COL = 16, 8   # x, dy and dx are column slices [COL, COL + C) of buffers C + PAD wide
TOL, TOL_DRES = (1e-3, 1e-4), (1e-4, 2e-5)   # (rtol, atol of the tensor's scale) against the fp64 formula; tests/test_gpu_bn_plan.py uses them too


def _close(got, ref, rtol, atol):
    got, ref = got.double().cpu().numpy(), ref.double().cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol * max(1.0, float(np.abs(ref).max())))


class _Slice:
    """Columns [COL, COL + C) of a (rows, C + PAD) buffer: .p / .ld for the C ABI, .v the strided view."""

    def __init__(self, rows, C, fill=None):
        self.t = torch.full((rows, C + PAD), 7.0, device="cuda")
        self.v = self.t[:, COL:COL + C]
        if fill is not None:
            self.v.copy_(fill)
        self.p, self.ld = self.t.data_ptr() + COL * 4, C + PAD


def _splits(rows, G):
    """Group boundaries inside a 32- / 34-row block of mopa_colsum's partition, at odd offsets (no multiple of any RL)."""
    a, b = {3922: (1301, 2711), 68000: (22667, 45011)}[rows]
    return [0, rows] if G == 1 else [0, a, rows] if G == 2 else [0, a, b, rows]


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


class _Case:
    """One (rows, C, G): inputs, the parent kernels' forward results and everything the checks share."""

    def __init__(self, rows, C, G):
        from mopa_amd._lib import call, load, ptr, query, stream
        self.call, self.ptr, self.query, self.stream, self.lib = call, ptr, query, stream, load()
        self.rows, self.C, self.G = rows, C, G
        self.b = _splits(rows, G)
        self.split = (self.b[1] if G > 1 else 0, self.b[2] if G > 2 else 0)
        g = torch.Generator(device="cuda").manual_seed(rows + 7 * C + G)
        rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
        self.x = _Slice(rows, C, rnd(rows, C) * 2 + 1)
        self.dy = _Slice(rows, C, rnd(rows, C))
        self.gamma, self.beta = torch.rand(C, device="cuda", generator=g) + 0.5, rnd(C)
        # channel 3: scale 0 and shift -0.0 (positive mean): x * 0 + (-0.0) is -0.0 for a negative x and +0.0 for a positive one, and
        # with a residual of -0.0 the pre-activation sums are exactly -0.0 and +0.0
        self.gamma[3], self.beta[3] = 0.0, -0.0
        self.res = rnd(rows, C)
        self.res[:, 3] = -0.0
        # ... and every 5th row of channels 8.. : residual = -(x * scale + shift) as the kernel rounds it, so the sum is exactly +0.0
        t0 = torch.empty(rows, C, device="cuda")
        self.fwd_parent(t0, torch.zeros(rows, C, device="cuda"), act=0)
        self.res[::5, 8:] = -t0[::5, 8:]
        self.y = torch.empty(rows, C, device="cuda")
        self.stats, self.rm, self.rv = self.fwd_parent(self.y, self.res, act=1)
        pre0 = int(((self.y == 0) & (self.res != 0)).sum())
        assert pre0 >= (rows // 5) * (C - 8) // 2, "the exact-zero sums were not hit"

    def _bn_common(self, rm, rv, stats, act, res):
        return (self.gamma.data_ptr(), self.beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), MOM, EPS, 0.0, act, res.data_ptr(), self.C, 1,
                stats.data_ptr())

    def fwd_parent(self, y, res, act):
        rm, rv, stats = torch.zeros(self.C, device="cuda"), torch.ones(self.C, device="cuda"), torch.empty(self.G, 4, self.C, device="cuda")
        ws = _ws(self.query("mopa_bnrelu_rows_workspace_bytes", self.rows, self.C))
        self.call("mopa_bn_act_fwd_groups", self.x.p, self.x.ld, y.data_ptr(), self.C, self.rows, self.C, self.G, *self.split,
                  *self._bn_common(rm, rv, stats, act, res), ws.data_ptr(), ws.numel(), self.stream())
        return stats, rm, rv

    def fwd_bits(self):
        y, bits = torch.empty(self.rows, self.C, device="cuda"), torch.zeros(self.rows, self.C // 32, dtype=torch.int32, device="cuda")
        rm, rv, stats = torch.zeros(self.C, device="cuda"), torch.ones(self.C, device="cuda"), torch.empty(self.G, 4, self.C, device="cuda")
        ws = _ws(self.query("mopa_bnrelu_rows_workspace_bytes", self.rows, self.C))
        self.call("mopa_bn_act_fwd_groups_bits", self.x.p, self.x.ld, y.data_ptr(), self.C, self.rows, self.C, self.G, *self.split,
                  *self._bn_common(rm, rv, stats, 1, self.res), 1, bits.data_ptr(), ws.data_ptr(), ws.numel(), self.stream())
        return y, stats, rm, rv, bits

    def bwd(self, dres0, acc_dres, residual=True, bits=None, colsum=False, parent=False):
        """-> dx, dres, dgamma, dbeta[, partial]: the parent's mopa_bn_act_bwd_groups (ymask = y) or the fused entry point."""
        dx = _Slice(self.rows, self.C)
        dres = dres0.clone() if residual else None
        dg, db = torch.full((self.C,), 0.25, device="cuda"), torch.full((self.C,), -0.5, device="cuda")   # accumulated into
        rp = (dres.data_ptr(), self.C, acc_dres) if residual else (None, 0, 0)
        head = (self.dy.p, self.dy.ld, self.x.p, self.x.ld, dx.p, dx.ld, self.rows, self.C, self.G, *self.split, self.stats.data_ptr(), 0.0, 1)
        if parent:
            ws = _ws(self.query("mopa_bnrelu_rows_bwd_workspace_bytes", self.rows, self.C))
            self.call("mopa_bn_act_bwd_groups", *head, self.y.data_ptr() if residual else None, self.C if residual else 0, *rp, 1,
                      dg.data_ptr(), db.data_ptr(), 1, 0, ws.data_ptr(), ws.numel(), self.stream())
            return dx, dres, dg, db
        ws = _ws(self.query("mopa_bn_act_bwd_groups_fused_workspace_bytes", self.rows, self.C))
        nblk = self.query("mopa_colsum_partial_blocks", self.rows)
        part = torch.full((nblk * self.C,), float("nan"), device="cuda") if colsum else None
        self.call("mopa_bn_act_bwd_groups_fused", *head, int(bits is not None), self.ptr(bits), *rp, 1, dg.data_ptr(), db.data_ptr(), 1, 0,
                  self.ptr(part), ws.data_ptr(), ws.numel(), self.stream())
        return dx, dres, dg, db, part

    def bias_grads(self, dx, part):
        """(mopa_colsum(dx), mopa_colsum_reduce(partials)) without and with accumulation."""
        out = []
        for acc in (0, 1):
            a, b = torch.full((self.C,), 0.375, device="cuda"), torch.full((self.C,), 0.375, device="cuda")
            ws = _ws(self.query("mopa_colsum_workspace_bytes", self.rows, self.C))
            self.call("mopa_colsum", dx.p, dx.ld, self.rows, self.C, a.data_ptr(), acc, ws.data_ptr(), ws.numel(), self.stream())
            self.call("mopa_colsum_reduce", part.data_ptr(), self.rows, self.C, b.data_ptr(), acc, self.stream())
            out.append((a, b))
        return out

    def reference(self, mask):
        """The fp64 formula on the given activation mask -> dx, dres, dgamma, dbeta (parameter gradients summed over the groups)."""
        x, dy, gm = self.x.v.double(), self.dy.v.double(), self.gamma.double()
        dz = dy * mask.double()
        dx, dgam, dbet = torch.empty_like(x), torch.zeros(self.C, dtype=torch.float64, device="cuda"), torch.zeros(self.C, dtype=torch.float64, device="cuda")
        for r0, r1 in zip(self.b[:-1], self.b[1:]):
            xs, zs = x[r0:r1], dz[r0:r1]
            mean, var = xs.mean(0), xs.var(0, unbiased=False)
            inv = 1.0 / torch.sqrt(var + EPS)
            xhat = (xs - mean) * inv
            dbet += zs.sum(0)
            dgam += (zs * xhat).sum(0)
            dx[r0:r1] = gm * inv * (zs - zs.mean(0) - xhat * (zs * xhat).mean(0))
        return dx, dz, dgam, dbet


_CASES = [(3922, C, G) for C in (64, 128, 256, 512) for G in (1, 2, 3)] + [(68000, 64, 3), (68000, 128, 2), (68000, 256, 1), (68000, 512, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C,G", _CASES)
def test_mask_bits_and_fused_column_sums_give_the_bits_of_the_existing_kernels(rows, C, G):
    """Kernel level, through the C ABI.  3,922 rows = 32-row blocks with a ragged tail, 68,000 = 34-row blocks (no multiple of RL);
    C = 64 .. 512 is RL = 16 .. 2; group boundaries inside a block at odd rows; x, dy, dx are column slices of wider buffers; residual
    gradient written and accumulated; pre-activation sums of exactly +0.0 and -0.0 among the inputs."""
    c = _Case(rows, C, G)
    # Part A, forward: same y, stats and running statistics; the bits are `y > 0`
    y, stats, rm, rv, bits = c.fwd_bits()
    assert torch.equal(y, c.y) and torch.equal(stats, c.stats) and torch.equal(rm, c.rm) and torch.equal(rv, c.rv)
    w = (bits.view(rows, C // 32, 1).long() >> torch.arange(32, device="cuda")) & 1
    assert torch.equal(w.view(rows, C).bool(), c.y > 0)
    assert torch.equal(c.fwd_bits()[4], bits)
    g = torch.Generator(device="cuda").manual_seed(1)
    dres0 = torch.randn(rows, C, device="cuda", generator=g)
    for acc_dres in (0, 1):
        pdx, pdres, pdg, pdb = c.bwd(dres0, acc_dres, parent=True)
        forms = {"bits": c.bwd(dres0, acc_dres, bits=bits), "bits + colsum": c.bwd(dres0, acc_dres, bits=bits, colsum=True),
                 "bits + colsum again": c.bwd(dres0, acc_dres, bits=bits, colsum=True)}
        for name, (dx, dres, dg, db, part) in forms.items():
            assert torch.equal(dx.t, pdx.t), (name, "dx")   # (the padding columns too: nothing written outside the slice)
            assert torch.equal(dres, pdres) and torch.equal(dg, pdg) and torch.equal(db, pdb), name
            if part is not None:
                for a, b in c.bias_grads(pdx, part):
                    assert torch.equal(a, b), (name, "column sums")
        assert torch.equal(forms["bits + colsum"][4], forms["bits + colsum again"][4])
    # Part B alone: no residual, mask recomputed from x (the decoder's BatchNorms)
    pdx, _, pdg, pdb = c.bwd(None, 0, residual=False, parent=True)
    runs = [c.bwd(None, 0, residual=False, colsum=True) for _ in range(2)]
    for dx, _, dg, db, part in runs:
        assert torch.equal(dx.t, pdx.t) and torch.equal(dg, pdg) and torch.equal(db, pdb)
        for a, b in c.bias_grads(pdx, part):
            assert torch.equal(a, b)
    assert torch.equal(runs[0][4], runs[1][4])
    # fp64: the fused forms against the formula (mask = the stored output's sign, the exact zeros have no sign in fp64)
    dx, dres, dg, db, part = c.bwd(dres0, 0, bits=bits, colsum=True)
    rdx, rdz, rdg, rdb = c.reference(c.y > 0)
    _close(dx.v, rdx, *TOL)
    _close(dres, rdz, *TOL_DRES)
    _close(dg - 0.25, rdg, *TOL)
    _close(db + 0.5, rdb, *TOL)
    bias = torch.zeros(C, device="cuda")
    c.call("mopa_colsum_reduce", part.data_ptr(), rows, C, bias.data_ptr(), 0, c.stream())
    # The column sums: the exact sum of a BatchNorm's dx over a group is 0, so the yardstick is the fp64 sum of the dx that was written,
    # and the bound the one of fp32 summation: every partial is a chain of at most ceil(rpb / RL) + RL additions (a thread's rows, then
    # the RL row lanes; the partials are added in double), each of which rounds by at most 2^-24 of the running sum <= sum |dx|.
    rpb, RL = -(-rows // c.query("mopa_colsum_partial_blocks", rows)), 256 // (C // 4)
    bound = 2.0 ** -24 * (-(-rpb // RL) + RL) * dx.v.double().abs().sum(0)
    assert bool(((bias.double() - dx.v.double().sum(0)).abs() <= bound).all())


def _net_run(monkeypatch, on, native, iters, defer_up=True):
    """Net2DSeg, training mode, bn_groups = 2, 4 images of 64 x 96, dropout on: logits of every pass, every parameter gradient of
    every pass, seg_logit_all, and the final buffers."""
    from mopa_amd import dense2d, synth
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d
    from mopa_amd.optim import FlatAdam
    monkeypatch.setattr(dense2d, "BN_MASK_BITS", on)
    monkeypatch.setattr(dense2d, "BN_COLSUM_FUSED", on)
    monkeypatch.setattr(dense2d, "DEFER_UP_BN", defer_up)
    monkeypatch.setattr(dense2d, "GRAPH_2D", False)
    monkeypatch.setattr(dense2d, "NATIVE_2D", native)
    for k in dense2d.GRAPH_STATS:
        dense2d.GRAPH_STATS[k] = 0
    src, trg = synth.make_batch(2, H=64, W=96), synth.make_batch(2, first=5, H=64, W=96)
    batch = {"img": torch.cat([src["img"], trg["img"]]), "img_indices": list(src["img_indices"]) + list(trg["img_indices"]), "bn_groups": 2}
    torch.manual_seed(11)
    m = build_model_2d(default_cfg())[0].cuda().train()
    m.output_all = True
    opt = FlatAdam(m.parameters(), lr=1e-3)
    calls = []
    inner = dense2d.call
    monkeypatch.setattr(dense2d, "call", lambda name, *a: (calls.append(name), inner(name, *a))[1])
    outs = []
    for it in range(iters):
        opt.zero_grad()
        o = m(batch)
        g = torch.Generator(device="cuda").manual_seed(it)
        sum((o[k] * torch.randn(o[k].shape, device="cuda", generator=g)).sum() for k in ("seg_logit", "seg_logit2", "seg_logit_all")).backward()
        outs += [o["seg_logit"].detach().clone(), o["seg_logit_all"].detach().clone()]
        outs += [p.grad.clone() for p in m.parameters()]
        opt.step()
    torch.cuda.synchronize()
    monkeypatch.setattr(dense2d, "call", inner)
    return outs + [b.clone() for b in m.buffers()], calls, dict(dense2d.GRAPH_STATS)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "native", "eager, materialised up-convolution BatchNorm"])
def test_network_with_both_switches_on_equals_both_off(monkeypatch, mode):
    """Both switches on against both off, bit for bit: eagerly (two iterations), with the native command list (four iterations: the first
    runs eagerly, the second records and replays, the third and fourth replay), and with the up-convolutions' BatchNorm written out (MOPA_DEFER_UP_BN=0)."""
    native = mode == "native"
    iters = 4 if native else 2
    off, calls_off, _ = _net_run(monkeypatch, False, native, iters, defer_up=not mode.endswith("BatchNorm"))
    on, calls_on, st = _net_run(monkeypatch, True, native, iters, defer_up=not mode.endswith("BatchNorm"))
    assert "mopa_bn_act_bwd_groups_fused" not in calls_off and "mopa_colsum_reduce" not in calls_off
    passes = 2 if native else iters   # (a replayed pass does not go through dense2d.call)
    assert calls_on.count("mopa_bn_act_fwd_groups_bits") == 16 * passes       # bn2 of the 16 BasicBlocks
    assert calls_on.count("mopa_colsum_reduce") == 7 * passes                 # 7 of the 8 biases; the 8th sums dfeat
    assert calls_on.count("mopa_colsum") == 1 * passes and calls_off.count("mopa_colsum") == 8 * passes
    if native:
        assert st["forward_replays"] == 3 and st["backward_replays"] == 3, st   # the recording call replays what it recorded
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(off, on)):
        assert torch.equal(a, b), i


def _lib():
    from mopa_amd import _lib
    return _lib.load()


def test_generated_abi_files_hold_the_new_entry_points():
    spec = importlib.util.spec_from_file_location("gen_header", os.path.join(ROOT, "mopa_amd", "csrc", "gen_header.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for path, text in gen.generate().items():
        with open(os.path.join(ROOT, path)) as f:
            assert f.read() == text, f"{path} is stale: run mopa_amd/csrc/gen_header.py"
        for name in ("mopa_bn_act_fwd_groups_bits", "mopa_bn_act_bwd_groups_fused", "mopa_colsum_reduce"):
            assert name in text, (path, name)


def test_bad_arguments_are_refused_before_any_launch():
    """No device is touched: the pointers are small non-null integers, a call that got past its checks would fault the process (and on
    a machine without a GPU fail with the launch error -3, not -1)."""
    lib = _lib()
    P, ws, ws_bytes = 4096, 4096, 1 << 30
    f = ctypes.c_float

    def fwd(C, leak, want, bits, res=P, act=1, training=1):
        return lib.mopa_bn_act_fwd_groups_bits(P, C, P, C, 64, C, 1, 0, 0, P, P, P, P, f(0.1), f(1e-5), f(leak), act, res, C if res else 0,
                                               training, P, want, bits, ws, ws_bytes, None)

    def bwd(C, leak, use, bits):
        return lib.mopa_bn_act_bwd_groups_fused(P, C, P, C, P, C, 64, C, 1, 0, 0, P, f(leak), 1, use, bits, P, C, 0, 1, P, P, 0, 0, None, ws,
                                                ws_bytes, None)

    assert fwd(48, 0.0, 1, P) == -1 and bwd(48, 0.0, 1, P) == -1          # C % 32 != 0
    assert fwd(64, 0.01, 1, P) == -1 and bwd(64, 0.01, 1, P) == -1        # a leak: the bit is not `y > 0`
    assert fwd(64, 0.0, 1, None) == -1 and bwd(64, 0.0, 1, None) == -1    # the flag without the pointer
    assert lib.mopa_bn_act_bwd_groups_fused(P, 64, P, 64, P, 64, 64, 64, 1, 0, 0, P, f(0.0), 1, 0, None, P, 64, 0, 1, P, P, 0, 0, None, ws,
                                            ws_bytes, None) == -1             # a residual gradient without bits
    assert fwd(64, 0.0, 1, P, res=None) == -1 and fwd(64, 0.0, 1, P, act=0) == -1 and fwd(64, 0.0, 1, P, training=0) == -1
    assert lib.mopa_colsum_reduce(None, 64, 64, P, 0, None) == -1 and lib.mopa_colsum_reduce(P, 64, 62, P, 0, None) == -1
    assert lib.mopa_colsum_partial_blocks(3922) == 123 and lib.mopa_colsum_partial_blocks(68000) == 2000
    assert lib.mopa_bn_act_bwd_groups_fused_workspace_bytes(3922, 64) == lib.mopa_bnrelu_rows_bwd_workspace_bytes(3922, 64)
