"""mopa_adam_flat leaves the bits it left before the update became a body shared with mopa_adam_flat_guarded.

tests/golden/adam_flat_bits.npy was recorded from the library as it was BEFORE that change: row 0-2 p, exp_avg, exp_avg_sq at
the start, rows 3-5 the gradients of three steps, rows 6-8 p, exp_avg, exp_avg_sq after them (n = 1203: 300 float4s and a scalar
tail of 3; weight decay 0.01, grad_scale 0.5).  Which products of the update fuse into an FMA decides the last bit, and a compiler
left to choose has chosen differently for the same source in another kernel: csrc/optim.hip writes the choice out, this pins it."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_flat_bits.npy")
N, STEPS = 1203, 3
SCALARS = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, gs=0.5)


def make_inputs():
    """(6, N) float32: p, exp_avg, exp_avg_sq and three gradients (what the recording script fed the library)."""
    rng = np.random.Generator(np.random.PCG64(2024))
    x = rng.standard_normal((3 + STEPS, N)).astype(np.float32)
    x[2] = np.abs(x[2]) * 1e-2
    return x


def run_steps(step_fn, inputs):
    """Three steps through `step_fn(p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale)` -> (3, N) host array."""
    f32 = lambda x: float(np.float32(x))
    buf = torch.from_numpy(np.ascontiguousarray(inputs[[0, 3, 1, 2]])).cuda()      # p, g, m, v: rows of 1203 floats are NOT 16-byte
    stride = (N + 3) // 4 * 4                                                      # aligned, so each gets a padded row of its own
    pad = torch.zeros(4, stride, device="cuda")
    pad[:, :N] = buf
    s = SCALARS
    for t in range(1, STEPS + 1):
        pad[1, :N] = torch.from_numpy(np.ascontiguousarray(inputs[2 + t])).cuda()
        step_fn(pad[0].data_ptr(), pad[1].data_ptr(), pad[2].data_ptr(), pad[3].data_ptr(), N, f32(s["lr"]), f32(s["b1"]), f32(s["b2"]),
                f32(s["eps"]), f32(s["wd"]), f32(1 - 0.9 ** t), f32(math.sqrt(1 - 0.999 ** t)), f32(s["gs"]))
    torch.cuda.synchronize()
    return pad[[0, 2, 3], :N].cpu().numpy()


def test_adam_flat_keeps_the_recorded_bits():
    from mopa_amd import _lib
    gold = np.load(GOLDEN)
    assert gold.shape == (9, N) and gold.dtype == np.float32
    inputs = gold[:6]
    want = gold[6:].view(np.int32)
    plain = run_steps(lambda *a: _lib.call("mopa_adam_flat", *a, _lib.stream()), inputs)
    for name, got, ref in zip(("p", "exp_avg", "exp_avg_sq"), plain.view(np.int32), want):
        assert np.array_equal(got, ref), f"mopa_adam_flat: {name} differs from the recorded bits in {int((got != ref).sum())} of {N} elements"
    rec = np.zeros(8, np.int32)
    rec.view(np.float32)[2] = 1.0
    rec[3] = 1
    rec = torch.from_numpy(rec).cuda()
    guarded = run_steps(lambda *a: _lib.call("mopa_adam_flat_guarded", *a, rec.data_ptr(), _lib.stream()), inputs)
    assert np.array_equal(guarded.view(np.int32), want), "mopa_adam_flat_guarded with coef 1 differs from the recorded bits"
