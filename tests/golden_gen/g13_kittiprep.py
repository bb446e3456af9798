"""Generate tests/golden/g13_kittiprep.npz and tests/golden/g13_kittiprep_fullsize.json by RUNNING the reference's SemanticKITTI
projection on the host: ``SemanticKITTISCN.preprocess`` and ``SemanticKITTIBase.select_points_in_frustum``
(mopa/data/semantic_kitti/semantic_kitti_dataloader.py:236-252,422-507), imported from the checkout (``torchvision``,
``torchsparse`` and the imports of the ``visualize`` module that are not installed are stubbed; ``np.bool8``, which this numpy no
longer has, is aliased), behind the extraction expressions of ``data_extraction`` (:349-371), which are stated here as
g11_scanprep.py states the datasets' expressions: they read files.

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixtures are what travels).
Usage, from the repo root:  python tests/golden_gen/g13_kittiprep.py PATH_TO_MOPA_CHECKOUT

While ``preprocess`` runs, ``np.matmul`` and ``np.around`` are wrapped so that the reference's own raw product and rounded points
are recorded.  The generator ASSERTS that the raw product equals, in every bit and on every point of both fixtures, the fused
chain ``fma(m3, 1, fma(m2, z, fma(m1, y, m0 * x)))`` (``fused_product``; ``fma32`` is a correctly rounded float32 fma in numpy) --
a BLAS that sums differently shows here, not on the GPU -- and that the rounded points equal ``rint(q * 100f) / 100f``.

The .npz holds ``meta`` (JSON: ``rows`` = the rows per block the sizes were chosen around, and one entry per case -- name, B,
image_size, pseudo, with_g, label dtype, counts) and per case ``k`` / sample ``b`` the inputs ``c<k>_s<b>_{scan, label, proj, g,
mask, img_in}``, the recorded intermediates ``_raw`` (Nf, 3) / ``_rounded`` (Nf, 2) over the front-half points, and the outputs
``_{points, feats, seg_labels, points_img, ori_keep_idx, g_indices, full_scan, all_seg_labels}``.  Cases: see ``small_cases``.
The .json holds position-weighted 64-bit checksums of every output of 4 scans of 120,000 points at 1226 x 370 (``fullsize_inputs``
and ``checksum``, which tests/test_gpu_kittiprep.py defines identically).
"""
import importlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "g13_kittiprep.npz")
OUT_FULL = os.path.join(ROOT, "tests", "golden", "g13_kittiprep_fullsize.json")
ROWS = 1024                     # csrc/kittiprep.hip KP_ROWS (tests/test_gpu_kittiprep.py asserts the library still says so)
F32 = np.float32


class _Stub(types.ModuleType):
    """A module that is not installed: every attribute is a class that accepts anything."""
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {"__init__": lambda self, *a, **k: None})


def _load(ref):
    sys.path.insert(0, ref)
    for name in ("torchvision", "torchvision.transforms", "torchsparse", "torchsparse.utils", "torchsparse.utils.quantize",
                 "torchsparse.utils.collate", "cv2", "matplotlib", "matplotlib.pyplot", "open3d", "pypatchworkpp"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _Stub(name)
    if not hasattr(np, "bool8"):
        np.bool8 = np.bool_
    mod = importlib.import_module("mopa.data.semantic_kitti.semantic_kitti_dataloader")
    assert os.path.realpath(mod.__file__).startswith(os.path.realpath(ref)), mod.__file__
    return mod


# ---------------------------------------------------------------------------- shared with tests/test_gpu_kittiprep.py
def checksum(a) -> int:
    """Position-weighted sum of the array's bytes modulo 2^64."""
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).astype(np.uint64)
    return int((b * np.arange(1, b.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


# KITTI odometry sequence 00, calib.txt: P2 and Tr (public calibration)
P2 = np.array([[718.856, 0, 607.1928, 45.38225], [0, 718.856, 185.2157, -0.1130887], [0, 0, 1, 0.003779761]])
TR = np.array([[4.276802385584e-04, -9.999672484946e-01, -8.084491683471e-03, -1.198459927713e-02],
               [-7.210626507497e-03, 8.081198471645e-03, -9.999413164504e-01, -5.403984729748e-02],
               [9.999738645903e-01, 4.859485810390e-04, -7.206933692422e-03, -2.921968648686e-01], [0, 0, 0, 1]])
KITTI_SIZE = (1226, 370)
FULL = dict(B=4, n=120000, seed=131)


def kitti_proj():
    """proj_matrix as the dataset's pickle holds it (float64; preprocess casts it to float32)."""
    return P2 @ TR


def lidar_cloud(rng, n):
    """A 140 m x 140 m cloud around the sensor, z from below the -3 m cut to 2 m: about half in front, about a fifth in the image."""
    return np.stack([rng.uniform(-70, 70, n), rng.uniform(-70, 70, n), rng.uniform(-3.4, 2, n), rng.random(n)], 1).astype(F32)


def raw_labels(rng, n):
    """The .label file viewed as int32: a semantic id in the low 16 bits (some with bit 15 set), an instance id above them (some
    with bit 31 set)."""
    sem = rng.integers(0, 260, n).astype(np.uint32)
    sem[rng.random(n) < 0.1] |= 0x8000
    inst = rng.integers(0, 1 << 16, n).astype(np.uint32)
    return ((inst << 16) | sem).view(np.int32)


def fullsize_inputs():
    rng = np.random.Generator(np.random.PCG64(FULL["seed"]))
    out = []
    for b in range(FULL["B"]):
        n = FULL["n"]
        out.append({"scan": lidar_cloud(rng, n), "label": raw_labels(rng, n), "proj": kitti_proj(),
                    "g": np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)})
    return out
# ---------------------------------------------------------------------------- end of the shared part


def fma32(a, b, c):
    """float32(a * b + c) rounded once, for float32 arrays: the product of two float32 is exact in float64; the float64 sum is
    made round-to-odd from its exact error (two-sum), and a round-to-odd value of 53 bits rounds to 24 bits as the exact sum does."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        other = np.nextafter(s, toward)
        even = (s.view(np.int64) & 1) == 0
        s = np.where(inexact & even, other, s)
    return s.astype(F32)


def fused_product(m, pts):
    """(n, 3): row r = fma(m[r,3], 1, fma(m[r,2], z, fma(m[r,1], y, m[r,0] * x))) in float32; m (3, 4) float32, pts (n, 3) float32."""
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    one = np.ones_like(x)
    out = np.empty((len(pts), 3), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            acc = (m[r, 0] * x).astype(F32)
            acc = fma32(np.full_like(x, m[r, 1]), y, acc)
            acc = fma32(np.full_like(x, m[r, 2]), z, acc)
            out[:, r] = fma32(np.full_like(x, m[r, 3]), one, acc)
    return out


def cents(q):
    """numpy's float32 np.around(q, 2)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.rint(q * F32(100)) / F32(100)


def same_bits(a, b):
    """Equal in every bit; a NaN equals a NaN (its sign and payload are not arithmetic)."""
    return a.shape == b.shape and a.dtype == b.dtype == F32 and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------- the reference
def extract(s):
    """data_extraction (:349-371) on the file contents: -> data_dict as preprocess receives it, and the z filter."""
    scan = s["scan"].reshape((-1, 4))
    points = scan[:, :3]
    feats = scan[:, 3]
    label = s["label"].view(np.uint32).reshape((-1)) if s["label"].dtype == np.int32 else s["label"].astype(np.uint32)
    label = label & 0xFFFF
    with np.errstate(invalid="ignore"):
        z_idx = points[:, 2] > -3
    points, feats, label = points[z_idx], feats[z_idx], label[z_idx]
    d = {"image": types.SimpleNamespace(size=tuple(s["size"])), "feats": feats, "points": points, "seg_labels": label.astype(np.int16),
         "all_seg_labels": label.astype(np.int16)}
    if "proj" in s:
        d["proj_matrix"] = s["proj"]
    if "g" in s:
        g_mask = np.zeros(scan.shape[0])
        g_mask[s["g"]] = 1
        d["g_indices"] = g_mask[z_idx].astype(np.bool8)
    if "mask" in s:
        nk = int(s["mask"].sum())
        d.update({"pseudo_label_2d": np.zeros(nk, np.int64), "pseudo_label_3d": np.zeros(nk, np.int64), "probs_2d": np.ones(nk, F32),
                  "probs_3d": np.ones(nk, F32), "ori_keep_idx": s["mask"], "ori_img_points": s["img_in"]})
    return d


def run_reference(mod, s):
    """extract + the reference's preprocess on one sample.  -> (outputs, recorded intermediates or None)."""
    d = extract(s)
    full_scan, all_seg = d["points"].copy(), d["all_seg_labels"].copy()
    obj = object.__new__(mod.SemanticKITTISCN)
    rec = {}
    matmul, around = np.matmul, np.around

    def rec_matmul(a, b, **kw):
        out = matmul(a, b, **kw)
        rec["m"], rec["h"], rec["raw"] = a, b.T, out.T
        return out

    def rec_around(a, **kw):
        out = around(a, **kw)
        rec["q"], rec["rounded"] = a, out
        return out

    np.matmul, np.around = rec_matmul, rec_around
    try:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            d = mod.SemanticKITTISCN.preprocess(obj, d)
    finally:
        np.matmul, np.around = matmul, around
    out = {"points": d["points"], "feats": d["feats"], "seg_labels": d["seg_labels"], "points_img": np.ascontiguousarray(d["points_img"]),
           "ori_keep_idx": d["ori_keep_idx"], "full_scan": full_scan, "all_seg_labels": all_seg}
    if "g" in s:
        out["g_indices"] = d["g_indices"]
    assert out["points"].dtype == F32 and out["feats"].dtype == F32 and out["feats"].shape == (len(out["points"]), 1)
    assert out["seg_labels"].dtype == np.int16 and out["ori_keep_idx"].dtype == np.bool_ and out["points_img"].dtype == F32
    if "mask" in s:
        assert not rec, "the pseudo-label form projects nothing"
        return out, None
    # the pin: this host's float32 BLAS product is the fused chain, on every point
    m32 = s["proj"].astype(F32)
    front = full_scan[full_scan[:, 0] > 0]
    assert same_bits(rec["m"], m32) and same_bits(np.ascontiguousarray(rec["h"][:, :3]), front) and rec["raw"].dtype == F32
    raw = np.ascontiguousarray(rec["raw"])
    chain = fused_product(m32, front)
    bad = ((raw.view(np.uint32) != chain.view(np.uint32)) & ~(np.isnan(raw) & np.isnan(chain))).any(1)
    if bad.any():
        raise SystemExit(f"numpy's float32 matmul on this host is NOT the fused chain on {int(bad.sum())} of {len(bad)} points: the fixture "
                         "would pin another arithmetic than csrc/kittiprep.hip computes")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = raw[:, :2] / raw[:, 2:3]
    assert same_bits(np.ascontiguousarray(rec["q"]), q)
    rounded = np.ascontiguousarray(rec["rounded"])
    assert same_bits(rounded, cents(q)), "np.around(q, 2) is not rint(q * 100f) / 100f on this host"
    return out, {"raw": raw, "rounded": rounded}


# ---------------------------------------------------------------------------- the small cases
def exact_matrix():
    """Small integers: with coordinates that are multiples of 1/8 every product and partial sum is exact in any order.
    u = (4 x - 8 y) / (x - 1), v = (2 x - 8 z) / (x - 1); image 16 x 8."""
    return np.array([[4, -8, 0, 0], [2, 0, -8, 0], [1, 0, 0, -1]], np.float64), (16, 8)


def exact_edges():
    """(x, y, z, what) placed exactly on every edge of the stage."""
    just_above = float(np.nextafter(F32(-3), F32(0)))
    return [
        (2, 1, 0, "u = 0: excluded"), (2, -1, 0, "u = 16 = W: excluded"), (2, 0, 0.5, "v = 0: excluded"), (2, 0, -0.5, "v = 8 = H: excluded"),
        (2, 0.875, 0.375, "u = 1, v = 1: kept"), (2, -0.875, -0.375, "u = 15, v = 7: kept"),
        (9, 4.375, 1.875, "u = 0.125 -> 12.5 -> 12 (even below), v = 0.375 -> 37.5 -> 38 (even above): kept"),
        (9, 3.375, 0.875, "u = 1.125 -> 112.5 -> 112, v = 1.375 -> 137.5 -> 138: kept"),
        (1, 0.5, 0.25, "depth 0, numerators 0: NaN, dropped"), (1, 0, 0, "depth 0, numerators > 0: +inf, dropped"),
        (1, 1, 1, "depth 0, numerators < 0: -inf, dropped"), (0.5, 0.5, 0.25, "depth -0.5: u = 4, v = 2, kept"),
        (0.5, 0, 0, "depth -0.5: u = -4, dropped"), (9, 0, -3, "z = -3 exactly: the z filter drops it (u = 4.5, v = 5.25 otherwise)"),
        (9, 0, just_above, "z just above -3: kept"), (0, 1, 0.5, "x = 0 exactly: not in the front half (u = 8, v = 4 otherwise)"),
        (-0.0, 1, 0.5, "x = -0"), (9, 0, float("nan"), "z NaN: the z filter drops it"), (float("nan"), 0, 0, "x NaN: not in the front half"),
        (9, float("nan"), 0, "y NaN: a NaN product, dropped by the frustum test"),
    ]


def dyadic_cloud(rng, n):
    q = np.stack([rng.integers(-40, 200, n) / 8, rng.integers(-160, 160, n) / 8, rng.integers(-32, 24, n) / 8, rng.integers(0, 256, n) / 256], 1)
    return q.astype(F32)


def small_cases():
    """-> list of (meta, samples).  R = ROWS.
    realistic    B = 3, N = R - 1, R, R + 1; real calibration, clouds that span the frustum edges; labels with bit 15 and with
                 high bits set; ground lists that hold the first and the last raw index
    sizes        B = 5, N = 2 R + 3, 0, 1, 300 with an empty front half (Nk = 0 between non-empty scans), 700; ground lists empty
                 (and necessarily empty for N = 0)
    all_kept     B = 2, every point lies in the image; int64 labels; no ground list
    exact        B = 3, the small-integer matrix with dyadic coordinates: every edge of ``exact_edges``, in the first block and
                 behind a block boundary, plus dyadic clouds; a ground list with a repeated and a negative (from the end) index
    pseudo       B = 2, the pseudo-label form: a loaded mask that no projection would give, loaded image points, ground lists
    """
    rng = np.random.Generator(np.random.PCG64(13))
    cases = []

    def add(name, samples, size, **kw):
        for s in samples:
            s["size"] = size
        cases.append((dict(name=name, B=len(samples), image_size=list(size), pseudo="mask" in samples[0], with_g="g" in samples[0],
                           label_dtype=str(samples[0]["label"].dtype), **kw), samples))

    def ground(n, k):
        g = np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
        g[0], g[-1] = 0, n - 1
        return g

    add("realistic", [dict(scan=lidar_cloud(rng, n), label=raw_labels(rng, n), proj=kitti_proj(), g=ground(n, n // 3))
                      for n in (ROWS - 1, ROWS, ROWS + 1)], KITTI_SIZE)
    sizes = []
    for j, n in enumerate((2 * ROWS + 3, 0, 1, 300, 700)):
        s = dict(scan=lidar_cloud(rng, n), label=raw_labels(rng, n), proj=kitti_proj(), g=np.zeros(0, np.int32))
        if j == 2:
            s["scan"][0, :3] = (20.0, 1.0, -0.5)                 # the one point is kept
        if j == 3:
            s["scan"][:, 0] = -np.abs(s["scan"][:, 0])
        sizes.append(s)
    add("sizes", sizes, KITTI_SIZE)
    kept = []
    for n in (ROWS + 1, 5):
        x = rng.uniform(15, 60, n)
        kept.append(dict(scan=np.stack([x, x * rng.uniform(-0.5, 0.5, n), rng.uniform(-1.7, -1.0, n) + x * 0.02, rng.random(n)], 1).astype(F32),
                         label=raw_labels(rng, n).view(np.uint32).astype(np.int64), proj=kitti_proj()))
    add("all_kept", kept, KITTI_SIZE)
    m, size = exact_matrix()
    edges = np.array([e[:3] + (0.5,) for e in exact_edges()], F32)
    a = np.concatenate([edges, dyadic_cloud(rng, ROWS - 7 - len(edges)), edges, dyadic_cloud(rng, 40)])   # the second set straddles row R
    exact = [dict(scan=a, label=raw_labels(rng, len(a)), proj=m, g=np.array([0, 5, 5, -2, len(a) - 1], np.int32)),
             dict(scan=dyadic_cloud(rng, 333), label=raw_labels(rng, 333), proj=m, g=ground(333, 100)),
             dict(scan=edges.copy(), label=raw_labels(rng, len(edges)), proj=m, g=np.zeros(0, np.int32))]
    add("exact", exact, size, edges=[e[3] for e in exact_edges()])
    pseudo = []
    for n in (ROWS + 77, 400):
        scan = lidar_cloud(rng, n)
        nz = int((scan[:, 2] > -3).sum())
        mask = rng.random(nz) < 0.3
        pseudo.append(dict(scan=scan, label=raw_labels(rng, n), mask=mask, g=ground(n, n // 4),
                           img_in=(rng.random((int(mask.sum()), 2)) * np.array([370, 1226])).astype(F32)))
    add("pseudo", pseudo, KITTI_SIZE)
    return cases


def main():
    mod = _load(sys.argv[1])
    assert mod.SemanticKITTISCN.select_points_in_frustum is mod.SemanticKITTIBase.select_points_in_frustum
    save, metas = {}, []
    for k, (meta, samples) in enumerate(small_cases()):
        counts = []
        for b, s in enumerate(samples):
            out, rec = run_reference(mod, s)
            for key in ("scan", "label", "proj", "g", "mask", "img_in"):
                if key in s:
                    save[f"c{k}_s{b}_{key}"] = s[key]
            for key, v in {**out, **(rec or {})}.items():
                save[f"c{k}_s{b}_{key}"] = np.asarray(v)
            counts.append([len(out["full_scan"]), len(out["points"])])
        meta["counts"] = counts
        metas.append(meta)
        print(k, meta["name"], "N", [len(s["scan"]) for s in samples], "[Nz, Nk]", counts)
    names = {m["name"]: m for m in metas}
    assert names["sizes"]["counts"][1] == [0, 0] and names["sizes"]["counts"][2] == [1, 1] and names["sizes"]["counts"][3][1] == 0
    assert all(c[0] == c[1] == n for c, n in zip(names["all_kept"]["counts"], (ROWS + 1, 5)))
    exact_keep = save[f"c{[m['name'] for m in metas].index('exact')}_s2_ori_keep_idx"]
    want = np.array(["kept" in e[3] for e in exact_edges() if not ("z = -3 exactly" in e[3] or "z NaN" in e[3])])
    assert np.array_equal(exact_keep, want), (exact_keep, want)
    save["meta"] = np.asarray(json.dumps({"rows": ROWS, "cases": metas}))
    np.savez_compressed(OUT, **save)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")

    full = {"kept": [], "nz": []}
    outs = []
    for s in fullsize_inputs():
        s["size"] = KITTI_SIZE
        out, _ = run_reference(mod, s)
        outs.append(out)
        full["nz"].append(len(out["full_scan"]))
        full["kept"].append(len(out["points"]))
    for key in outs[0]:
        full[key] = checksum(np.concatenate([o[key].astype(np.uint8) if o[key].dtype == np.bool_ else o[key] for o in outs]))
    print("fullsize [Nz]", full["nz"], "[Nk]", full["kept"])
    with open(OUT_FULL, "w") as f:
        json.dump(full, f, indent=1, sort_keys=True)
    print("wrote", OUT_FULL)


if __name__ == "__main__":
    main()
