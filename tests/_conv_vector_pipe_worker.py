"""Worker of tests/test_gpu_conv_tiles.py::test_vector_pipe_kernels_in_a_child_process.

MOPA_CONV2D_MFMA is read once per process, so the vector-pipe kernels (k_conv2d_igemm<256,64>, <128,128>, <128,64>, <64,64>;
k_conv2d_wgrad<64,3>, <64,1>, <16,2>, <16,1>) need a process of their own: run with MOPA_CONV2D_MFMA=0 this script puts every
operator geometry of tests/_convgeom_reference.py through mopa_conv2d_igemm at the four tile overrides and every weight-gradient
case through mopa_conv2d_bwd_weight, against the float64 restatement under the bounds of tests/test_gpu_2d.py::_close, checks that
mopa_conv2d_igemm_classes refuses, prints the worst error per kernel and exits non-zero on any failure.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _convgeom_reference as cr  # noqa: E402
from _conv_tiles_gpu import (TILES, WORST, check_igemm, check_wgrad, igemm_expect, initial_out, report, run_igemm,  # noqa: E402
                             wgrad_kernel)


def main():
    if os.environ.get("MOPA_CONV2D_MFMA", "1") != "0":
        print("run with MOPA_CONV2D_MFMA=0: this worker is the vector-pipe kernels' test", file=sys.stderr)
        return 2
    failures = []
    for case in cr.igemm_cases():
        P = cr.problem(*case)
        cout = cr.fields(P.geoms[0]).Cout
        for accumulate in (False, True):
            init = initial_out(P, accumulate)
            ref, mask = igemm_expect(P, init, accumulate)
            for tile in range(4):
                try:
                    if tile == 1 and cout % 128:
                        try:
                            run_igemm(P, tile, accumulate, init)
                            failures.append(f"{P.name}: the 128x128 tile took {cout} output channels")
                        except RuntimeError:
                            pass
                        continue
                    check_igemm(f"k_conv2d_igemm<{TILES[tile]}>", P, run_igemm(P, tile, accumulate, init), init, ref, mask)
                except AssertionError as e:
                    failures.append(str(e))
    for case in cr.wgrad_cases():
        P = cr.problem(*case)
        try:
            check_wgrad(wgrad_kernel(P, False), P)
        except AssertionError as e:
            failures.append(str(e))
    P = cr.problem("convt", (2, 3, 5), 64, 64, True)
    try:
        run_igemm(P, None, False, initial_out(P, False), classes=True)
        failures.append("mopa_conv2d_igemm_classes ran on the vector pipe")
    except RuntimeError:
        pass
    torch.cuda.synchronize()
    report()
    want = {f"k_conv2d_igemm<{t}>" for t in TILES} | {f"k_conv2d_wgrad<{v}>" for v in ("64,3", "64,1", "16,2", "16,1")}
    if set(WORST) != want:
        failures.append(f"kernels run: {sorted(WORST)}")
    for f in failures:
        print("FAILED", f, file=sys.stderr, flush=True)
    print(f"[conv tiles] vector pipe: {len(failures)} failures", flush=True)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
