"""Fixture G13 (tests/golden_gen/g13_kittiprep.py: the reference's SemanticKITTI preprocess run on the host) is what
csrc/kittiprep.hip states it is -- the recorded float32 BLAS product is the fused chain, the recorded rounding is
rint(q * 100f) / 100f -- and every argument check of mopa_amd/kittiprep.py names its key before anything is launched.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


@pytest.fixture(scope="module")
def g13():
    g = np.load(os.path.join(GOLDEN, "g13_kittiprep.npz"))
    return g, json.loads(str(g["meta"]))


def fma32(a, b, c):
    """float32(a * b + c) rounded once: the product of two float32 is exact in float64; the float64 sum is made round-to-odd from
    its exact error (two-sum), and a round-to-odd value of 53 bits rounds to 24 bits as the exact sum does."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        s = np.where(inexact & ((s.view(np.int64) & 1) == 0), other, s)
    return s.astype(F32)


def fused_product(m, pts):
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty((len(pts), 3), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            acc = (m[r, 0] * x).astype(F32)
            acc = fma32(np.full_like(x, m[r, 1]), y, acc)
            acc = fma32(np.full_like(x, m[r, 2]), z, acc)
            out[:, r] = fma32(np.full_like(x, m[r, 3]), np.ones_like(x), acc)
    return out


def same_bits(a, b):
    """Equal in every bit; a NaN equals a NaN."""
    return a.shape == b.shape and a.dtype == b.dtype == F32 and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_fma32_rounds_once():
    """The helper against exact rational arithmetic, on sums that a float64 intermediate would round twice."""
    from fractions import Fraction
    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.standard_normal(4000).astype(F32)
    b = rng.standard_normal(4000).astype(F32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 3, 4000)).astype(F32)
    # a * b = 2^-24 - 2^-70, c = 1 + 2^-23: the exact sum lies just below a tie of the float32 grid, the float64 sum ON it (and
    # would round to even, upwards); mirrored in sign
    a[:2] = [F32(2.0 ** -24 * (1 + 2.0 ** -23)), F32(-(2.0 ** -24) * (1 + 2.0 ** -23))]
    b[:2] = F32(1 - 2.0 ** -23)
    c[:2] = [F32(1 + 2.0 ** -23), F32(-(1 + 2.0 ** -23))]
    got = fma32(a, b, c)
    assert got[0] == F32(1 + 2.0 ** -23) and got[1] == -got[0]
    assert F32(np.float64(a[0]) * np.float64(b[0]) + np.float64(c[0])) == F32(1 + 2.0 ** -22)      # what rounding twice gives
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F32(float(exact))                  # float(Fraction) and float32(float) could round twice: pick the nearest of lo's neighbours exactly
        cands = [lo, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)


def test_fixture_loads(g13):
    g, meta = g13
    assert meta["rows"] == 1024
    names = [c["name"] for c in meta["cases"]]
    assert names == ["realistic", "sizes", "all_kept", "exact", "pseudo"]
    R = meta["rows"]
    ns = {len(g[f"c{k}_s{b}_scan"]) for k, c in enumerate(meta["cases"]) for b in range(c["B"])}
    assert {R - 1, R, R + 1, 2 * R + 3, 0, 1} <= ns
    for k, c in enumerate(meta["cases"]):
        for b in range(c["B"]):
            nz, nk = c["counts"][b]
            p = f"c{k}_s{b}_"
            assert g[p + "scan"].dtype == F32 and g[p + "scan"].shape[1] == 4 and g[p + "label"].dtype == np.dtype(c["label_dtype"])
            assert g[p + "points"].shape == (nk, 3) and g[p + "feats"].shape == (nk, 1) and g[p + "points_img"].shape == (nk, 2)
            assert g[p + "seg_labels"].shape == (nk,) and g[p + "seg_labels"].dtype == np.int16
            assert g[p + "ori_keep_idx"].shape == (nz,) and g[p + "ori_keep_idx"].dtype == np.bool_ and int(g[p + "ori_keep_idx"].sum()) == nk
            assert g[p + "full_scan"].shape == (nz, 3) and g[p + "all_seg_labels"].shape == (nz,)
            assert (p + "g_indices" in g.files) == c["with_g"] and (p + "mask" in g.files) == c["pseudo"]
    sizes = meta["cases"][names.index("sizes")]["counts"]
    assert sizes[1] == [0, 0] and sizes[3][0] > 0 and sizes[3][1] == 0 and sizes[2][1] > 0 and sizes[4][1] > 0    # Nk = 0 between non-empty scans
    assert all(nz == nk for nz, nk in meta["cases"][names.index("all_kept")]["counts"])
    k = names.index("realistic")
    lab = np.concatenate([g[f"c{k}_s{b}_label"] for b in range(3)])
    assert (lab & 0x8000).any() and (lab < 0).any() and (g[f"c{k}_s0_seg_labels"] < 0).any()       # bit 15, bit 31, a wrapped int16
    assert g[f"c{k}_s0_g"][0] == 0 and g[f"c{k}_s0_g"][-1] == len(g[f"c{k}_s0_scan"]) - 1
    assert len(g[f"c{names.index('sizes')}_s0_g"]) == 0


def _projected(g, meta):
    for k, c in enumerate(meta["cases"]):
        if not c["pseudo"]:
            for b in range(c["B"]):
                yield k, b, c


def test_recorded_product_is_the_fused_chain(g13):
    g, meta = g13
    seen = 0
    for k, b, c in _projected(g, meta):
        scan = g[f"c{k}_s{b}_scan"]
        z = scan[scan[:, 2] > -3]
        front = z[z[:, 0] > 0][:, :3]
        raw = g[f"c{k}_s{b}_raw"]
        assert raw.shape == (len(front), 3)
        assert same_bits(raw, fused_product(g[f"c{k}_s{b}_proj"].astype(F32), front)), (k, b)
        seen += len(front)
    assert seen > 4000


def test_exact_case_is_exact_in_any_order(g13):
    """The small-integer matrix with dyadic coordinates: the float64 product, rounded, is the recorded one (no sum rounds)."""
    g, meta = g13
    k = [c["name"] for c in meta["cases"]].index("exact")
    for b in range(meta["cases"][k]["B"]):
        scan = g[f"c{k}_s{b}_scan"]
        z = scan[scan[:, 2] > -3]
        front = z[z[:, 0] > 0]
        h = np.concatenate([front[:, :3], np.ones((len(front), 1), F32)], 1).astype(np.float64)
        with np.errstate(invalid="ignore"):
            exact = h @ g[f"c{k}_s{b}_proj"].T
        assert same_bits(g[f"c{k}_s{b}_raw"], exact.astype(F32))


def test_recorded_rounding_is_rint_of_cents(g13):
    g, meta = g13
    ties = 0
    for k, b, c in _projected(g, meta):
        raw = g[f"c{k}_s{b}_raw"]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            q = raw[:, :2] / raw[:, 2:3]
            cents = q * F32(100)
            want = np.rint(cents) / F32(100)
            ties += int((np.abs(cents - np.trunc(cents)) == 0.5).sum())
        assert same_bits(g[f"c{k}_s{b}_rounded"], want), (k, b)
        # and the outputs are these points: the strict frustum test, the fliplr
        w, h = c["image_size"]
        with np.errstate(invalid="ignore"):
            keep = (want[:, 0] > 0) & (want[:, 1] > 0) & (want[:, 0] < w) & (want[:, 1] < h)
        assert same_bits(g[f"c{k}_s{b}_points_img"], np.ascontiguousarray(want[keep][:, ::-1]))
    assert ties >= 8                                            # both parities, twice per scan of the exact case that has them


def _sample(n=5, **over):
    s = {"scan": torch.zeros(n, 4), "label": torch.zeros(n, dtype=torch.int32), "proj_matrix": np.zeros((3, 4), np.float32)}
    s.update(over)
    return {k: v for k, v in s.items() if v is not ...}


def test_argument_checks_name_the_key():
    from mopa_amd.kittiprep import prepare_scans_kitti as run
    size = (1226, 370)
    with pytest.raises(ValueError, match="no samples"):
        run([], size)
    with pytest.raises(RuntimeError, match="scan must be on the GPU .*no CPU fallback"):
        run([_sample()], size)
    for bad in ((0, 370), (1226,), None, (1226, -1)):
        with pytest.raises(ValueError, match="image_size"):
            run([_sample()], bad)
    with pytest.raises(TypeError, match="scan of sample 0 must be a torch tensor"):
        run([_sample(scan=np.zeros((5, 4), np.float32))], size)
    with pytest.raises(TypeError, match="scan must be float32"):
        run([_sample(scan=torch.zeros(5, 4, dtype=torch.float64))], size)
    with pytest.raises(ValueError, match=r"scan of sample 1 must be \(N, 4\)"):
        run([_sample(), _sample(scan=torch.zeros(5, 3))], size)
    with pytest.raises(TypeError, match="label of sample 0 must be a torch tensor"):
        run([_sample(label=...)], size)
    with pytest.raises(TypeError, match="label must be int32"):
        run([_sample(label=torch.zeros(5, dtype=torch.int16))], size)
    with pytest.raises(ValueError, match=r"label of sample 0 must be \(5,\)"):
        run([_sample(label=torch.zeros(4, dtype=torch.int32))], size)
    with pytest.raises(TypeError, match="label must have one dtype per call"):
        run([_sample(), _sample(label=torch.zeros(5, dtype=torch.int64))], size)
    with pytest.raises(TypeError, match="proj_matrix of sample 0 must be a numpy array"):
        run([_sample(proj_matrix=torch.zeros(3, 4))], size)
    with pytest.raises(TypeError, match="proj_matrix of sample 0"):
        run([_sample(proj_matrix=...)], size)
    with pytest.raises(ValueError, match=r"proj_matrix of sample 0 must be a \(3, 4\) float array"):
        run([_sample(proj_matrix=np.zeros((4, 4), np.float32))], size)
    with pytest.raises(ValueError, match="proj_matrix of sample 0"):
        run([_sample(proj_matrix=np.zeros((3, 4), np.int64))], size)
    g = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="every sample of a call has `g_indices` or none"):
        run([_sample(g_indices=g), _sample()], size)
    with pytest.raises(TypeError, match="g_indices must be int32"):
        run([_sample(g_indices=g.long())], size)
    with pytest.raises(ValueError, match=r"g_indices of sample 0 must be \(G,\)"):
        run([_sample(g_indices=g.reshape(1, 2))], size)
    keep, pts = torch.zeros(5, dtype=torch.bool), torch.zeros(0, 2)
    with pytest.raises(ValueError, match="every sample of a call has `ori_keep_idx` or none"):
        run([_sample(ori_keep_idx=keep, ori_img_points=pts), _sample()], size)
    with pytest.raises(ValueError, match="`ori_keep_idx` and `ori_img_points` come together"):
        run([_sample(ori_keep_idx=keep)], size)
    with pytest.raises(TypeError, match="ori_keep_idx must be bool"):
        run([_sample(ori_keep_idx=keep.to(torch.uint8), ori_img_points=pts)], size)
    with pytest.raises(ValueError, match=r"ori_keep_idx of sample 0 must be \(Nz,\)"):
        run([_sample(ori_keep_idx=keep.reshape(5, 1), ori_img_points=pts)], size)
    with pytest.raises(TypeError, match="ori_img_points must be float32"):
        run([_sample(ori_keep_idx=keep, ori_img_points=pts.double())], size)
    with pytest.raises(ValueError, match=r"ori_img_points of sample 0 must be \(Nk, 2\)"):
        run([_sample(ori_keep_idx=keep, ori_img_points=torch.zeros(0, 3))], size)
    # the pseudo-label form needs no matrix; what is left is the device
    with pytest.raises(RuntimeError, match="scan must be on the GPU"):
        run([_sample(ori_keep_idx=keep, ori_img_points=pts, proj_matrix=...)], size)
