"""Generate tests/golden/g15_nuscprep.npz and tests/golden/g15_nuscprep_fullsize.json by RUNNING the reference's nuScenes projection
on the host: ``map_pointcloud_to_image`` (mopa/data/nuscenes/projection.py:9-90), imported from the checkout.  The two libraries
it imports are not installed: ``pyquaternion.Quaternion`` and ``nuscenes.utils.geometry_utils.view_points`` are stood in for by
``rotation_matrix_numpy`` and ``view_points`` of tests/_nuscenes_reference.py, written from the libraries' published definitions
(UNVERIFIED against the libraries); matplotlib is stubbed.  ``preprocess()`` itself needs a NuScenes database object, so its
labelling loop (preprocess.py:116-126) and the devkit's ``points_in_box`` are stated (``paint_labels``), as g13_kittiprep.py states
``data_extraction``.

TEST INFRASTRUCTURE ONLY; never runs on the GPU box (the committed fixtures are what travels).
Usage, from the repo root:  python tests/golden_gen/g15_nuscprep.py PATH_TO_MOPA_CHECKOUT

While the reference runs, its ``@`` products (through an ndarray subclass whose ``__rmatmul__`` records) and every ``np.dot`` of the
stand-ins are recorded.  The generator ASSERTS, on every point of every small case, that
  * every recorded 2-D product is per element the fused chain fma(a[K-1], b[K-1], ... fma(a1, b1, a0 * b0)) (K = 3: the four
    rotations, the box corners; K = 4: the quaternion product, viewpad), and every 1-D . 1-D dot (q.q, dot(i,i)) likewise;
  * the elementwise restatement (tests/_nuscenes_reference.py::preprocess_scan, exact fma) equals what the reference left, in
    every bit of the mask, points_img and the labels;
  * the 1-D . 2-D ``np.dot(i, v)`` of points_in_box -- which on this host is NOT one fixed chain over all N (the body of the loop is
    fma(i0, v0, i1 * v1) + i2 * v2, its tail is the fully fused chain) -- stays farther than 1e-9 * dot(i,i) from both bounds on
    every point of every box, so that the labels do not depend on the order; in the ``exact`` case, where every product and sum
    is exact in any order, that it equals the device's chain instead.
A BLAS that sums differently shows here, not on the GPU.

The .npz holds ``meta`` (JSON: ``rows``, ``lds_boxes`` and one entry per case: name, B, image_size, ground form, counts) and per
case ``k`` / sample ``b`` the inputs ``c<k>_s<b>_{scan, calib, boxes, box_class, g, gmask}`` (calib packed as
``_nuscenes_reference.pack_calib``) and the outputs ``_{points, points_img, seg_labels, valid_mask, proj_matrix, g_indices}``.
The .json holds G13's position-weighted checksums of every output of ``fullsize_inputs`` (4 sweeps of 34,720 points at 1600 x 900
with 40 boxes each), produced through numpy's fast path after the small cases have pinned it; the margin to the box faces is asserted
on every kept point of these sweeps too, before the file is written.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _nuscenes_reference as ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g15_nuscprep.npz")
OUT_FULL = os.path.join(ROOT, "tests", "golden", "g15_nuscprep_fullsize.json")
ROWS = 1024                     # csrc/nuscprep.hip NP_ROWS      (tests/test_gpu_nuscprep.py asserts the library still says so)
LDS_BOXES = 64                  # csrc/nuscprep.hip NP_LDS_BOXES
F32 = np.float32
REC = []                        # recorded products: (a, b, out)
# N1: numpy multiplies the (3, 1) cloud of a ONE-point sweep as matrix x VECTOR (gemv), which on this host sums a row in another
# order than the chain (the reference itself gives a point other float64 intermediates alone than inside a larger sweep).  The
# device computes the chain whatever N is.  Single-column products are therefore only held to the chain within rounding, and the
# one-point sweep is pinned by its outputs alone: mask, float32 image point and label equal the restatement's in every bit.
N1_RANGE = 20.0


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {"__init__": lambda self, *a, **k: None})


class Rec(np.ndarray):
    """The point cloud as the reference receives it: ``R @ pc`` lands in __rmatmul__ (a subclass's reflected operator goes first)."""
    def __rmatmul__(self, other):
        a, b = np.asarray(other), np.asarray(self)
        out = np.matmul(a, b)
        REC.append((a.copy(), b.copy(), out.copy()))
        return out.view(Rec)


_dot = np.dot


def rec_dot(a, b):
    out = _dot(a, b)
    REC.append((np.array(a), np.array(b), np.array(out)))
    return out


def _load(checkout):
    sys.path.insert(0, checkout)
    quat = types.ModuleType("pyquaternion")

    class Quaternion:
        def __init__(self, q):
            self.q = np.array(q, dtype=float)
        rotation_matrix = property(lambda self: ref.rotation_matrix_numpy(self.q))
    quat.Quaternion = Quaternion
    geo = types.ModuleType("nuscenes.utils.geometry_utils")
    geo.view_points = ref.view_points
    sys.modules.update({"pyquaternion": quat, "nuscenes": types.ModuleType("nuscenes"), "nuscenes.utils": types.ModuleType("nuscenes.utils"),
                        "nuscenes.utils.geometry_utils": geo})
    for name in ("matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _Stub(name)
    mod = importlib.import_module("mopa.data.nuscenes.projection")
    assert os.path.realpath(mod.__file__).startswith(os.path.realpath(checkout)), mod.__file__
    return mod


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    iv = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((a.view(iv) == b.view(iv)) | (np.isnan(a) & np.isnan(b))).all())


def assert_chains(what):
    """Every recorded product against the fused chain, then the record is cleared."""
    bad = total = 0
    for a, b, out in REC:
        a, b = a.astype(np.float64), b.astype(np.float64)
        if a.ndim == 1 and b.ndim == 1:
            total += 1
            bad += not same_bits(np.float64(out), np.float64(ref.chain(a, b)))
        elif a.ndim == 2 and b.ndim == 2:
            want = np.array([[ref.chain(a[r], b[:, c]) for c in range(b.shape[1])] for r in range(a.shape[0])]).reshape(out.shape)
            if b.shape[1] == 1:                          # matrix x vector (gemv): see N1 above; the outputs are still compared in every bit
                assert (np.abs(out - want) <= 4e-16 * (np.abs(a) @ np.abs(b))).all()
                continue
            total += out.size
            bad += int((~((out == want) | (np.isnan(out) & np.isnan(want)))).sum())
        # 1-D . 2-D: points_in_box's dot(i, v), see check_box_margins
    REC.clear()
    if bad:
        raise SystemExit(f"{what}: numpy's float64 products on this host are NOT the fused chain on {bad} of {total} elements: the fixture "
                         "would pin another arithmetic than csrc/nuscprep.hip computes")
    return total


def check_box_margins(what, pts, boxes, exact):
    """points_in_box's dot(i, v) on the kept points (3, Nk): far from both bounds, or (exact case) equal to the device's chain."""
    for box in boxes:
        corners = ref.box_corners(box)
        p1 = corners[:, 0]
        v = pts - p1.reshape((-1, 1))
        for col in (4, 1, 3):
            i = corners[:, col] - p1
            iv, ii = _dot(i, v), _dot(i, i)
            if exact:
                want = np.array([ref.chain(i, v[:, n]) for n in range(v.shape[1])])
                if not (iv == want.reshape(iv.shape)).all():          # by value: the sign of a zero decides no comparison
                    raise SystemExit(f"{what}: the exact case's dot(i, v) is not exact on this host")
            else:
                with np.errstate(invalid="ignore"):
                    near = np.minimum(np.abs(iv), np.abs(iv - ii)) <= 1e-9 * ii
                if near.any():
                    raise SystemExit(f"{what}: {int(near.sum())} points lie within 1e-9 dot(i,i) of a face of a box: their label could "
                                     "follow the order of the sum; choose another seed")


def run_reference(mod, s, size, what, exact=False):
    """The reference's projection + the stated labelling on one sample, with every assertion of the docstring."""
    scan, calib = s["scan"], s["calib"]
    kw = {k: s[k] for k in ("g", "g_mask") if k in s}
    proj = {}

    def project(pts, im_shape, info):
        mask, _, img, mtx = mod.map_pointcloud_to_image(pts.view(Rec), im_shape, info)
        proj["m"] = np.asarray(mtx)
        return np.asarray(mask), np.asarray(img)

    np.dot = rec_dot
    try:
        out = ref.preprocess_scan_numpy(scan, calib, s["boxes"], s["box_class"], size, project=project, **kw)
    finally:
        np.dot = _dot
    out["proj_matrix"] = proj["m"]
    assert sum(1 for r in REC if r[0].shape == (3, 3) and r[1].shape == (3, len(scan))) >= 4, what      # the four rotations were seen
    elements = assert_chains(what)
    check_box_margins(what, out["points"].T, s["boxes"], exact)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mine = ref.preprocess_scan(scan, calib, s["boxes"], s["box_class"], size, **kw)
    for key, v in mine.items():
        if not same_bits(v, out[key]):
            raise SystemExit(f"{what}: the elementwise restatement's {key} differs from what the reference left")
    assert out["points"].dtype == F32 and out["points_img"].dtype == F32 and out["seg_labels"].dtype == np.uint8 and out["valid_mask"].dtype == np.bool_
    return out, elements


# ---------------------------------------------------------------------------- the small cases
def exact_calib():
    """Identity, half-turn and third-turn quaternions (all entries of the matrices are 0 or +-1 exactly), dyadic translations, a
    small integer intrinsic: with dyadic coordinates every product and sum is exact in any order.  Camera axes: x = -ego y,
    y = -ego z, z = ego x.  u = 8 xc / zc + 8, v = 8 yc / zc + 4; image 16 x 8."""
    d = dict(zip(ref.CALIB_KEYS, ([1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1], [0.5, -0.5, 0.5, -0.5],
                                  [1, 0, 2], [1024, 512, 0], [1024.5, 512, 0], [1.5, 0, 1.5], [[8, 0, 8], [0, 8, 4], [0, 0, 1]])))
    return ref.unpack_calib(ref.pack_calib(d)), (16, 8)


def to_lidar(calib, cam):
    """Camera coordinates (n, 3) -> lidar coordinates; exact for the exact calibration."""
    R = [ref.rotation_matrix_numpy(calib[k]) for k in ref.CALIB_KEYS[:4]]
    t = [np.array(calib[k], dtype=np.float64) for k in ref.CALIB_KEYS[4:8]]
    p = np.asarray(cam, dtype=np.float64).T
    p = R[0].T @ (R[1].T @ (R[2] @ (R[3] @ p + t[3][:, None]) + t[2][:, None] - t[1][:, None]) - t[0][:, None])
    out = p.T.astype(F32)
    assert (out.astype(np.float64) == p.T).all(), "the exact case's lidar coordinates must be float32"
    return out


EXACT_BOX_CAM = (0.0, 0.0, 4.0)                 # the exact case's box: its centre in camera coordinates; wlh = (1, 2, 1), class 3


def exact_edges(calib):
    """-> (lidar xyz (n, 3) float32, [(what, kept, label)])."""
    e = 2.0 ** -18
    cam = [((-2, 0, 2), "u = 0: excluded", 0), ((2, 0, 2), "u = 16 = W: excluded", 0), ((0, -1, 2), "v = 0: excluded", 0),
           ((0, 1, 2), "v = 8 = H: excluded", 0), ((-2 + e, 0, 2), "u = 2^-16: kept", 1), ((2 - e, 0, 2), "u = 16 - 2^-16: kept", 1),
           ((0, -1 + e, 2), "v = 2^-16: kept", 1), ((0, 1 - e, 2), "v = 8 - 2^-16: kept", 1), ((0, 0, 0), "depth 0, numerators 0: NaN, dropped", 0),
           ((1, 1, 0), "depth 0, numerators > 0: +inf, dropped", 0), ((-1, -1, 0), "depth 0, numerators < 0: -inf, dropped", 0),
           ((0, 0, -2), "depth -2: u = 8, v = 4 lie in the image, dropped by depth > 0", 0)]
    pts = to_lidar(calib, [c[0] for c in cam])
    notes = [(c[1], bool(c[2]), ref.NO_BOX) for c in cam]
    c = to_lidar(calib, [EXACT_BOX_CAM])[0].astype(np.float64)
    up = lambda v: float(np.nextafter(F32(v), F32(np.inf)))
    down = lambda v: float(np.nextafter(F32(v), F32(-np.inf)))
    box_pts = [((c[0] + 1, c[1], c[2]), "on a face of the box: inside", 3), ((c[0] + 1, c[1] + 0.5, c[2]), "on an edge: inside", 3),
               ((c[0] + 1, c[1] + 0.5, c[2] + 0.5), "on a corner: inside", 3), ((c[0] - 1, c[1] - 0.5, c[2] - 0.5), "on the opposite corner: inside", 3),
               ((up(c[0] + 1), c[1], c[2]), "one float32 step outside in x", ref.NO_BOX), ((c[0], down(c[1] - 0.5), c[2]), "one step outside in y", ref.NO_BOX),
               ((c[0], c[1], up(c[2] + 0.5)), "one step outside in z", ref.NO_BOX), ((down(c[0] - 1), c[1] - 0.5, c[2] - 0.5), "one step off the corner", ref.NO_BOX)]
    pts = np.concatenate([pts, np.array([b[0] for b in box_pts], F32), np.array([[np.nan, 1, 1]], F32)])
    notes += [(b[1], True, b[2]) for b in box_pts] + [("a NaN coordinate: dropped", False, ref.NO_BOX)]
    return pts, notes


def rows5(rng, xyz):
    n = len(xyz)
    return np.concatenate([xyz, rng.integers(0, 256, (n, 1)).astype(F32), rng.integers(0, 32, (n, 1)).astype(F32)], 1).astype(F32)


def dyadic_cloud(rng, calib, n):
    cam = np.stack([rng.integers(-48, 48, n) / 8, rng.integers(-24, 24, n) / 8, rng.integers(-16, 64, n) / 8], 1)
    return to_lidar(calib, cam)


def small_cases():
    """-> list of (meta, samples).  R = ROWS; see the issue's list in the module docstring of tests/test_gpu_nuscprep.py."""
    rng = np.random.Generator(np.random.PCG64(15))
    cases = []

    def add(name, samples, size, **kw):
        ground = "g_indices" if "g" in samples[0] else "g_mask" if "g_mask" in samples[0] else None
        cases.append((dict(name=name, B=len(samples), image_size=list(size), ground=ground, **kw), samples))

    # realistic: N = R - 1, R, R + 1; 12 boxes: 1 and 2 overlap with different classes, 3 has no class and covers labelled points
    real = []
    for j, n in enumerate((ROWS - 1, ROWS, ROWS + 1)):
        calib = ref.nusc_calib(rng, raw_quaternion=1 if j == 0 else None)
        boxes, cls = ref.view_boxes(rng, calib, 12)
        boxes[1, 3:6] = [3.0, 6.0, 2.4]
        boxes[2] = boxes[1]
        boxes[2, :3] += [1.5, 1.2, 0.3]
        boxes[3] = boxes[1]
        boxes[3, 3:6] *= 1.3
        cls[1], cls[2], cls[3] = 4, 7, -1
        real.append(dict(scan=ref.lidar_sweep(rng, n, boxes), calib=calib, boxes=boxes, box_class=cls))
    add("realistic", real, ref.NUSC_SIZE)

    # sizes: N = 2 R + 3 (no boxes), 0, 1 (kept, in its box), 300 behind the camera, 700 with one box more than an LDS chunk
    sizes = []
    for j, (n, m) in enumerate(((2 * ROWS + 3, 0), (0, 3), (1, 1), (300, 2), (700, LDS_BOXES + 1))):
        calib = ref.nusc_calib(rng)
        boxes, cls = ref.view_boxes(rng, calib, m)
        scan = ref.lidar_sweep(rng, n, boxes, near=0.7 if j == 4 else 0.4)
        fwd, right, o = ref.camera_axis(calib)
        if j == 2:
            scan[0, :3] = o + fwd * N1_RANGE
            boxes[0, :3], cls[0] = scan[0, :3].astype(np.float64) + [0.3, -0.2, 0.1], 6
        if j == 3:
            scan[:, :3] = (o - fwd * rng.uniform(3, 40, (n, 1)) + rng.normal(0, 1.0, (n, 3))).astype(F32)
        if j == 4:
            cls[-1] = 9                                  # the box beyond the chunk labels something (asserted below)
            boxes[-1, 3:6] = [6.0, 9.0, 3.0]
        sizes.append(dict(scan=scan, calib=calib, boxes=boxes, box_class=cls))
    add("sizes", sizes, ref.NUSC_SIZE)

    # exact: every edge, in the first block and straddling row R
    calib, size = exact_calib()
    edges, notes = exact_edges(calib)
    centre = to_lidar(calib, [EXACT_BOX_CAM])[0].astype(np.float64)
    box = np.array([[*centre, 1, 2, 1, 1, 0, 0, 0], [*centre, 8, 8, 8, 1, 0, 0, 0]], np.float64)      # the second: no class, covers the first
    cls = np.array([3, -1])
    a = np.concatenate([edges, dyadic_cloud(rng, calib, ROWS - 7 - len(edges)), edges, dyadic_cloud(rng, calib, 40)])
    exact = [dict(scan=rows5(rng, a), calib=calib, boxes=box, box_class=cls),
             dict(scan=rows5(rng, dyadic_cloud(rng, calib, 333)), calib=calib, boxes=box, box_class=cls),
             dict(scan=rows5(rng, edges), calib=calib, boxes=box, box_class=cls)]
    add("exact", exact, size, edges=[n[0] for n in notes])

    # ground: an index list with the first and the last raw index, a repeat and a negative index; an empty list; the mask form
    gi, gm = [], []
    for j, n in enumerate((ROWS + 9, 400)):
        calib = ref.nusc_calib(rng)
        boxes, cls = ref.view_boxes(rng, calib, 4)
        scan = ref.lidar_sweep(rng, n, boxes)
        g = np.concatenate([[0, n - 1, 5, 5, -2], rng.choice(n, n // 3, replace=False)]).astype(np.int32) if j == 0 else np.zeros(0, np.int32)
        gi.append(dict(scan=scan, calib=calib, boxes=boxes, box_class=cls, g=g))
        gm.append(dict(scan=scan[:, :4].copy(), calib=calib, boxes=boxes, box_class=cls, g_mask=rng.random(n) < 0.4))   # (N, 4) rows too
    add("ground_idx", gi, ref.NUSC_SIZE)
    add("ground_mask", gm, ref.NUSC_SIZE)
    return cases, notes


def main():
    mod = _load(sys.argv[1])
    save, metas, elements = {}, [], 0
    cases, notes = small_cases()
    for k, (meta, samples) in enumerate(cases):
        counts = []
        for b, s in enumerate(samples):
            out, el = run_reference(mod, s, tuple(meta["image_size"]), f"{meta['name']}[{b}]", exact=meta["name"] == "exact")
            elements += el
            p = f"c{k}_s{b}_"
            save[p + "scan"], save[p + "calib"] = s["scan"], ref.pack_calib(s["calib"])
            save[p + "boxes"], save[p + "box_class"] = np.asarray(s["boxes"], np.float64).reshape(-1, 10), np.asarray(s["box_class"], np.int64)
            if "g" in s:
                save[p + "g"] = s["g"]
            if "g_mask" in s:
                save[p + "gmask"] = s["g_mask"]
            for key, v in out.items():
                save[p + key] = np.asarray(v)
            counts.append(int(len(out["points"])))
        meta["counts"] = counts
        metas.append(meta)
        print(k, meta["name"], "N", [len(s["scan"]) for s in samples], "M", [len(s["boxes"]) for s in samples], "Nk", counts,
              "labelled", [int((save[f"c{k}_s{b}_seg_labels"] != ref.NO_BOX).sum()) for b in range(len(samples))])
    names = [m["name"] for m in metas]
    # what the cases were built for
    k = names.index("realistic")
    for b in range(3):
        seg, pts, boxes = save[f"c{k}_s{b}_seg_labels"], save[f"c{k}_s{b}_points"].T, save[f"c{k}_s{b}_boxes"]
        in1, in2, in3 = (ref.points_in_box(boxes[j], pts) for j in (1, 2, 3))
        later = np.zeros(len(seg), bool)
        for j in range(4, 12):
            later |= ref.points_in_box(boxes[j], pts)
        assert (in1 & in2 & ~later).any() and (seg[in1 & in2 & ~later] == 7).all(), "the later of two overlapping boxes wins"
        assert (in1 & ~in2 & in3 & ~later).any() and (seg[in1 & ~in2 & in3 & ~later] == 4).all(), "a box without a class erases nothing"
    k = names.index("sizes")
    assert metas[k]["counts"][1] == 0 and metas[k]["counts"][2] == 1 and metas[k]["counts"][3] == 0 and metas[k]["counts"][0] > 0
    assert (save[f"c{k}_s0_seg_labels"] == ref.NO_BOX).all() and save[f"c{k}_s2_seg_labels"].tolist() == [6]
    last = ref.points_in_box(save[f"c{k}_s4_boxes"][-1], save[f"c{k}_s4_points"].T)
    assert last.any() and (save[f"c{k}_s4_seg_labels"][last] == 9).all(), "the box beyond the LDS chunk labels its points"
    k = names.index("exact")
    keep = save[f"c{k}_s2_valid_mask"]
    assert keep.tolist() == [n[1] for n in notes], [(n[0], bool(v)) for n, v in zip(notes, keep) if n[1] != v]
    assert save[f"c{k}_s2_seg_labels"].tolist() == [n[2] for n in notes if n[1]]
    first = save[f"c{k}_s0_valid_mask"]
    assert first[:len(notes)].tolist() == keep.tolist() and first[ROWS - 7:ROWS - 7 + len(notes)].tolist() == keep.tolist()
    k = names.index("ground_idx")
    assert save[f"c{k}_s0_g_indices"].any() and not save[f"c{k}_s1_g_indices"].any()
    save["meta"] = np.asarray(json.dumps({"rows": ROWS, "lds_boxes": LDS_BOXES, "cases": metas}))
    np.savez_compressed(OUT, **save)
    print("chains asserted on", elements, "elements; wrote", OUT, os.path.getsize(OUT), "bytes")

    def project(pts, im_shape, info):
        mask, _, img, _ = mod.map_pointcloud_to_image(pts, im_shape, info)
        return mask, img

    outs = []
    for b, s in enumerate(ref.fullsize_inputs()):
        outs.append(ref.preprocess_scan_numpy(s["scan"], s["calib"], s["boxes"], s["box_class"], ref.NUSC_SIZE, g=s["g"], project=project))
        # the labels of the full-size sweeps come from numpy's own dot(i, v): they equal the device's only away from the faces
        check_box_margins(f"fullsize[{b}]", outs[-1]["points"].T, s["boxes"], exact=False)
    full = {"kept": [int(len(o["points"])) for o in outs], "labelled": [int((o["seg_labels"] != ref.NO_BOX).sum()) for o in outs]}
    for key in outs[0]:
        full[key] = ref.checksum(np.concatenate([o[key].astype(np.uint8) if o[key].dtype == np.bool_ else o[key] for o in outs]))
    print("fullsize Nk", full["kept"], "labelled", full["labelled"], "-- no kept point within 1e-9 dot(i,i) of a box face (asserted on", sum(full["kept"]), "points)")
    with open(OUT_FULL, "w") as f:
        json.dump(full, f, indent=1, sort_keys=True)
    print("wrote", OUT_FULL)


if __name__ == "__main__":
    main()
