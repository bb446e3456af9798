"""SHA-256 digests of the raw output bytes of the grouped BatchNorm entry points of csrc/rows.hip, on fixed inputs.

Recorded on the commit BEFORE the partial-sum kernels became one templated body (round 13) and kept in tests/bn_parent_bits.json;
tests/test_gpu_bn_bits.py calls digests() and asserts equality.  The equality tests elsewhere compare one entry point with another,
and both sides now come from one template: a changed order of additions would pass them and not this.

    python profiles/bn_parent_bits.py [out.json]      (default: tests/bn_parent_bits.json; needs the GPU)

Shapes: 3,922 rows (32-row blocks with a ragged tail, group boundaries inside a block at odd rows), C = 64 .. 512 (RL = 16 .. 2),
1 .. 3 groups; x, dy, dx are column slices of wider buffers, whose padding columns are hashed with them.  The pool case: the
pre-pool maps of tests/test_gpu_stem_bwd.py::POOL_SHAPES, fresh and accumulating."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20261018
ROWS, SPLITS = 3922, (1301, 2711)
CASES = [(C, G) for C in (64, 128, 256, 512) for G in (1, 2, 3)]
POOL_SHAPES = [(1, 5, 7, 1), (2, 40, 56, 2), (3, 27, 45, 3)]
PAD, COL = 16, 8   # a slice: columns [COL, COL + C) of a (rows, C + PAD) buffer filled with 7.0
EPS, MOM = 1e-5, 0.1


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


class _Slice:
    def __init__(self, rows, C, fill=None):
        self.t = torch.full((rows, C + PAD), 7.0, device="cuda")
        if fill is not None:
            self.t[:, COL:COL + C] = fill
        self.p, self.ld = self.t.data_ptr() + COL * 4, C + PAD


def _bytes(n):
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device="cuda")


def _groups_case(out, C, G):
    from mopa_amd._lib import call, ptr, query, stream
    rng = np.random.Generator(np.random.PCG64([SEED, C, G]))
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda()   # noqa: E731
    rows = ROWS
    split = (SPLITS[0] if G > 1 else 0, SPLITS[1] if G > 2 else 0)
    x, dy = _Slice(rows, C, rnd(rows, C) * 2 + 1), _Slice(rows, C, rnd(rows, C))
    gamma, beta, res, dres0 = rnd(C).abs() + 0.5, rnd(C), rnd(rows, C), rnd(rows, C)
    tag = f"C{C}_G{G}"

    def fwd(bits):
        y = torch.empty(rows, C, device="cuda")
        rm, rv, stats = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.empty(G, 4, C, device="cuda")
        ws = _bytes(query("mopa_bnrelu_rows_workspace_bytes", rows, C))
        head = (x.p, x.ld, ptr(y), C, rows, C, G, *split, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), MOM, EPS, 0.0, 1, ptr(res), C, 1, ptr(stats))
        if bits is None:
            call("mopa_bn_act_fwd_groups", *head, ptr(ws), ws.numel(), stream())
        else:
            call("mopa_bn_act_fwd_groups_bits", *head, 1, ptr(bits), ptr(ws), ws.numel(), stream())
        return y, stats, rm, rv

    y, stats, rm, rv = fwd(None)
    out[f"fwd_groups/{tag}"] = _sha(y, stats, rm, rv)
    bits = torch.zeros(rows, C // 32, dtype=torch.int32, device="cuda")
    yb, statsb, _, _ = fwd(bits)
    out[f"fwd_groups_bits/{tag}"] = _sha(yb, statsb, bits)

    def bwd(name, fused, mask, use_bits=False, colsum=False, residual=True, acc_dres=0):
        dx = _Slice(rows, C)
        dres = dres0.clone() if residual else None
        dg, db = torch.full((C,), 0.25, device="cuda"), torch.full((C,), -0.5, device="cuda")   # accumulated into
        rp = (ptr(dres), C, acc_dres) if residual else (None, 0, 0)
        head = (dy.p, dy.ld, x.p, x.ld, dx.p, dx.ld, rows, C, G, *split, ptr(stats), 0.0, 1)
        outs = [dx.t, dg, db] + ([dres] if residual else [])
        if not fused:
            ws = _bytes(query("mopa_bnrelu_rows_bwd_workspace_bytes", rows, C))
            call("mopa_bn_act_bwd_groups", *head, ptr(y) if mask else None, C if mask else 0, *rp, 1, ptr(dg), ptr(db), 1, 0, ptr(ws),
                 ws.numel(), stream())
        else:
            ws = _bytes(query("mopa_bn_act_bwd_groups_fused_workspace_bytes", rows, C))
            part = torch.zeros(query("mopa_colsum_partial_blocks", rows) * C, device="cuda") if colsum else None
            call("mopa_bn_act_bwd_groups_fused", *head, int(use_bits), ptr(bits) if use_bits else None, *rp, 1, ptr(dg), ptr(db), 1, 0,
                 ptr(part), ptr(ws), ws.numel(), stream())
            outs += [part] if colsum else []
        out[f"{name}/{tag}"] = _sha(*outs)

    bwd("bwd_groups_ymask", False, True, acc_dres=1)
    bwd("bwd_groups_nomask", False, False)
    bwd("bwd_fused_bits", True, False, use_bits=True, acc_dres=1)
    bwd("bwd_fused_bits_colsum", True, False, use_bits=True, colsum=True)
    bwd("bwd_fused_colsum", True, False, colsum=True, residual=False)

    dgb, coef = torch.full((2, C), 0.25, device="cuda"), torch.empty(G, 2, C, device="cuda")
    ws = _bytes(query("mopa_bnrelu_rows_workspace_bytes", rows, C))
    call("mopa_bn_bwd_sums_groups", dy.p, dy.ld, x.p, x.ld, rows, C, G, *split, ptr(stats), 0.0, 1, None, 0, ptr(dgb), ptr(dgb, C), 1,
         ptr(coef), ptr(ws), ws.numel(), stream())
    out[f"bwd_sums/{tag}"] = _sha(dgb, coef)


def _pool_case(out, B, H, W, G, acc_dy):
    from mopa_amd._lib import call, ptr, query, stream
    rng = np.random.Generator(np.random.PCG64([SEED, B, H, W, acc_dy]))
    rnd = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).cuda()   # noqa: E731
    rows, OH, OW = B * H * W, (H + 1) // 2, (W + 1) // 2
    stats = torch.stack([rnd(G, 64), rnd(G, 64) * 0.5, rnd(G, 64) * 0.3, rnd(G, 64).abs() + 0.5], 1).contiguous()   # scale, shift, mean, 1 / std
    x = rnd(rows, 64)
    pooled, amax = torch.empty(B * OH * OW, 64, device="cuda"), torch.empty(B * OH * OW * 64, dtype=torch.uint8, device="cuda")
    call("mopa_maxpool3x3s2_fwd_bn", ptr(x), 64, B, H, W, 64, ptr(stats), G, ptr(pooled), 64, ptr(amax), stream())
    dpool, dy = rnd(B * OH * OW, 64), rnd(rows, 128)   # dy: the left half of a 128-wide buffer
    dgb, coef = torch.full((2, 64), 0.25, device="cuda"), torch.empty(G, 2, 64, device="cuda")
    ws = _bytes(query("mopa_bnrelu_rows_workspace_bytes", rows, 64))
    call("mopa_bn_bwd_sums_groups_pool", ptr(dpool), 64, ptr(amax), B, H, W, ptr(dy), 128, acc_dy, ptr(x), 64, 64, G, ptr(stats), 0.0, 1,
         ptr(dgb), ptr(dgb, 64), 1, ptr(coef), ptr(ws), ws.numel(), stream())
    out[f"bwd_sums_pool/{B}x{H}x{W}_G{G}_acc{acc_dy}"] = _sha(dy, dgb, coef, amax)


def digests():
    out = {}
    for C, G in CASES:
        _groups_case(out, C, G)
    for B, H, W, G in POOL_SHAPES:
        for acc_dy in (0, 1):
            _pool_case(out, B, H, W, G, acc_dy)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "bn_parent_bits.json")
    d = digests()
    assert d == digests(), "two runs on the same inputs differ"
    with open(path, "w") as f:
        json.dump({"seed": SEED, "digests": d}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(d)} digests -> {path}")
