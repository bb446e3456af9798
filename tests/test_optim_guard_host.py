"""The host side of FlatAdam's gradient guard (mopa_amd/optim.py): the chunk table of mopa_grad_stats, the unchanged checkpoint
layout, GradStats.summary.  No GPU: the kernels are in tests/test_gpu_optim_guard.py."""
import pytest
import torch

from mopa_amd.optim import FlatAdam, GradStats, stat_chunks

CHUNK = 8192


def guard_lengths(chunk):
    """Parameter lengths around every boundary of the table: below / at / above one float4, one chunk, many chunks, and 300
    tiny parameters (more parameters than a block has threads)."""
    return [1, 2, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 65 * chunk + 3] + [1 + i % 7 for i in range(300)]


def _slices(lengths):
    """(offset, numel) as FlatAdam lays parameters out: every one padded to a multiple of 4."""
    out, off = [], 0
    for n in lengths:
        out.append((off, n))
        off += (n + 3) // 4 * 4
    return out, off


@pytest.mark.parametrize("chunk", (CHUNK, 8, 4))
def test_stat_chunks_cover_every_parameter_exactly_once(chunk):
    lengths = guard_lengths(chunk)
    slices, total = _slices(lengths)
    chunks = stat_chunks(slices, chunk)
    owner = [-1] * total                      # parameter of every flat element, -1 = padding
    for i, (off, n) in enumerate(slices):
        owner[off:off + n] = [i] * n
    seen = [0] * total
    last = -1
    for p, lo, hi in chunks:
        assert 0 < hi - lo <= chunk and lo % 4 == 0
        assert p >= last, "records are sorted by parameter"
        last = p
        off, n = slices[p]
        assert off <= lo and hi <= off + n, "a chunk crosses its parameter (or reaches into the padding behind it)"
        for k in range(lo, hi):
            seen[k] += 1
    for k in range(total):
        assert seen[k] == (1 if owner[k] >= 0 else 0), (k, owner[k], seen[k])
    assert sum(hi - lo for _, lo, hi in chunks) == sum(lengths)
    assert len(chunks) == sum((n + chunk - 1) // chunk for n in lengths)


def test_stat_chunks_refuses_what_the_kernel_cannot_read():
    with pytest.raises(ValueError):
        stat_chunks([(0, 8)], 6)              # float4 loads: the chunk length is a multiple of 4
    with pytest.raises(ValueError):
        stat_chunks([(0, 8)], 0)
    with pytest.raises(ValueError):
        stat_chunks([(0, 3), (3, 5)], 8)      # a parameter that does not start on a float4
    assert stat_chunks([(0, 0), (0, 4)], 8) == [(1, 0, 4)]   # an empty parameter has no chunk


def test_chunk_table_matches_the_library():
    """The chunk length is the library's compile-time constant (pure host query)."""
    from mopa_amd import _lib
    chunk = _lib.query("mopa_grad_stats_chunk")
    assert chunk == CHUNK and chunk % 4 == 0
    assert _lib.query("mopa_grad_stats_workspace_bytes", 100) >= 100 * 16


def _params():
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s)) for s in ((3, 5), (7,), (2, 2, 2))]


def test_guard_arguments_leave_the_checkpoint_layout_alone():
    plain = FlatAdam(_params(), lr=1e-3, weight_decay=0.01)
    guarded = FlatAdam(_params(), lr=1e-3, weight_decay=0.01, max_grad_norm=2.5, skip_nonfinite=True)
    assert guarded.max_grad_norm == 2.5 and guarded.skip_nonfinite is True and guarded.last_stats is None
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False
    a, b = plain.state_dict(), guarded.state_dict()
    assert a.keys() == b.keys() and a["state"] == b["state"] == {}
    assert [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    assert "max_grad_norm" not in b["param_groups"][0] and "skip_nonfinite" not in b["param_groups"][0]
    for opt in (plain, guarded):              # ... and with moments in it (t > 0)
        opt.t = 3
    a, b = plain.state_dict(), guarded.state_dict()
    assert a["state"].keys() == b["state"].keys() and all(a["state"][i].keys() == b["state"][i].keys() for i in a["state"])
    ref = torch.optim.Adam(_params(), lr=1e-3, weight_decay=0.01)
    ref.load_state_dict(b)                    # torch's own Adam takes the guarded optimizer's checkpoint
    guarded.load_state_dict(ref.state_dict())
    assert guarded.t == 3 and guarded.max_grad_norm == 2.5 and guarded.skip_nonfinite is True
    with pytest.raises(ValueError):
        FlatAdam(_params(), max_grad_norm=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        guarded.grad_stats()


def test_summary_names_the_largest_and_the_non_finite():
    st = GradStats(torch.tensor(float("nan")), torch.tensor(2, dtype=torch.int32), torch.tensor([0.5, float("nan"), 3.0, 1.0]),
                   torch.tensor([0.1, 0.2, 0.3, 0.4]), torch.tensor([0, 2, 0, 0], dtype=torch.int32),
                   coef=torch.tensor(1.0), applied=torch.tensor(0, dtype=torch.int32), n_skipped=torch.tensor(4), n_clipped=torch.tensor(1))
    line = st.summary(names=["a", "b", "c", "d"], top=2)
    assert "largest: b nan, c 3" in line and ", d " not in line and "a 0.5" not in line
    assert "non-finite in: b (2)" in line and "SKIPPED" in line and "skipped 4, clipped 1" in line
    plain = GradStats(torch.tensor(2.0), torch.tensor(0, dtype=torch.int32), torch.tensor([2.0]), torch.tensor([1.5]),
                      torch.tensor([0], dtype=torch.int32))
    assert plain.summary() == "grad norm 2; non-finite 0; largest: #0 2"
