"""Worker of tests/test_gpu_spconv_kernels.py::test_wide_pipelined_kernels_in_a_child_process.

MOPA_SPCONV_PATH is read once per process, and k_spconv_pipe<2,6,32>, <3,6,40> and <4,4,28> exist only behind MOPA_SPCONV_PATH=1: run
with it, this script launches them through mopa_spconv_fwd_grouped on the 27-offset tables of `mixed` and `block8` (tests/_spconv_cases.py)
at 32, 48 and 64 output channels and one, three and five input chunks, with the assertions of the parent test -- the query names the
kernel, float64 accuracy under the forward bounds, untouched sentinels, the same bits on a second launch -- prints the worst error
per kernel and exits non-zero on any failure."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import _spconv_cases as C  # noqa: E402


def main():
    if os.environ.get("MOPA_SPCONV_PATH") != "1":
        print("run with MOPA_SPCONV_PATH=1: this worker is the wide pipelined kernels' test", file=sys.stderr)
        return 2
    import torch
    bench = C.Bench3D()
    failures = []
    for cout, want in ((16, "k_spconv_pipe<1,2,40>"), (32, "k_spconv_pipe<2,6,32>"), (48, "k_spconv_pipe<3,6,40>"), (64, "k_spconv_pipe<4,4,28>")):
        vecs = []
        for cin in (16, 48, 80):
            case = (1, 27, 0, cin, cout, 1, 0, 0)   # packed weights, no stated size: the switch alone selects the kernel
            for name in ("mixed", "block8"):
                for kind, level, flip in C.tables_of(name, 27):
                    for transposed in (False, True):
                        kname, v = bench.measure(case, name, kind, level, flip, transposed)
                        if kname != want:
                            failures.append(f"{case} on {name}: the query names {kname}, not {want}")
                        vecs.append(v)
        m = torch.stack(vecs).cpu().numpy()
        print(f"{want}: {len(m)} launches, worst error {m[:, 0].max():.3f} of the bound, {m[:, 1].max():.2e} of max|ref|, "
              f"bits equal to the dense-table kernel's in {int((m[:, 4] == 1).sum())} of {len(m)}")
        if not (m[:, 0] <= 1).all():
            failures.append(f"{want}: error {m[:, 0].max():.3f} x the bound")
        if not (m[:, 2] == 1).all():
            failures.append(f"{want}: wrote outside its slice")
        if not (m[:, 3] == 1).all():
            failures.append(f"{want}: a second launch gave other bits")
    for f in failures:
        print("FAIL", f)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
