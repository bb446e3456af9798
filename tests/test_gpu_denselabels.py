"""Dense 2D pseudo labels on the device (mopa_amd.imageprep.prepare_dense_pslabels, csrc/denselabels.hip) against fixture G17 --
what the reference's own refine_sam_2Dlabels produced on the host (tests/golden_gen/g17_denselabels.py) -- and against the numpy
restatement (tests/_denselabels_reference.py) on random inputs.  Every input is asserted to have no undecided id, so every comparison
is an equality over all pixels.  Reads only the committed fixtures."""
import json
import os

import numpy as np
import pytest
import torch

import _denselabels_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g17_denselabels.npz")))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(samples, C=10, windows=None, flip=None, **kw):
    from mopa_amd import imageprep as ip
    return ip.prepare_dense_pslabels([dev(s["probs"]) for s in samples], [dev(s["labels"]) for s in samples],
                                     [dev(s["points"]) for s in samples], [dev(s["mask"]) for s in samples], num_classes=C,
                                     windows=windows, flip=flip, **kw)


def expected(s, C=10, window=None, flip=False, thre=0.1):
    out, undecided = ref.dense_pslabels(s["probs"], s["labels"], s["points"], s["mask"], C, thre, window, flip, return_undecided=True)
    assert undecided == [], f"undecided ids {undecided}: choose another seed"
    return out


def sample(seed, *args, **kw):
    return ref.random_sample(np.random.Generator(np.random.PCG64(seed)), *args, **kw)


def test_every_fixture_case_matches_exactly(g):
    for k in range(int(g["n"])):
        s = {key: g[f"c{k}_{key}"] for key in ("probs", "labels", "points", "mask")}
        window = tuple(int(v) for v in g[f"c{k}_window"])
        window, flip = (None if window[0] < 0 else window), bool(g[f"c{k}_flip"])
        out = run([s], windows=None if window is None else [window], flip=[flip])
        assert out.dtype == torch.int32 and np.array_equal(out[0].cpu().numpy(), g[f"c{k}_out"]), f"case {k}"


def test_full_size_batches_equal_the_recorded_checksums(golden_dir):
    with open(os.path.join(golden_dir, "g17_denselabels_fullsize.json")) as f:
        want = json.load(f)
    samples = ref.fullsize_inputs()
    plain = run(samples).cpu().numpy()
    crop = run(samples, windows=[s["window"] for s in samples], flip=[s["flip"] for s in samples]).cpu().numpy()
    assert list(plain.shape) == want["shape_plain"] and list(crop.shape) == want["shape_crop_flip"]
    assert int((plain == -100).sum()) == want["n_ignored_plain"] and int((crop == -100).sum()) == want["n_ignored_crop_flip"]
    assert ref.checksum(plain) == want["plain"] and ref.checksum(crop) == want["crop_flip"]


# the smallest shapes that can go wrong: 8 x 8 cells; an odd width (row tails, rows at every store alignment); points and pixels
# over several workgroups; 300 points on 16 pixels (every pixel fought over)
SHAPES = {"cells": dict(H=24, W=40, n=120, cell=8, ids=14, big_rows=5),
          "odd": dict(H=23, W=37, n=110, cell=6, ids=20),
          "blocks": dict(H=72, W=130, n=700, cell=9, ids=100, big_rows=12),
          "patch": dict(H=24, W=40, n=300, cell=8, ids=14, patch=(9, 17, 4, 4))}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_random_inputs_equal_the_restatement(name):
    s = sample(20 + sorted(SHAPES).index(name), **SHAPES[name])
    H, W = s["mask"].shape
    want = expected(s)
    a = run([s])
    assert np.array_equal(a[0].cpu().numpy(), want)
    assert torch.equal(a, run([s]))                                          # run to run
    window = (3, 2, W - 2, H - 1)                                            # an odd left origin; the width keeps W's parity
    for flip in (False, True):
        out = run([s], windows=[window], flip=[flip])
        assert np.array_equal(out[0].cpu().numpy(), expected(s, window=window, flip=flip)), (name, flip)


def test_a_batch_of_unequal_point_counts_with_an_empty_sample():
    ss = [sample(31, 24, 40, 150, 8, 14, big_rows=5), sample(32, 24, 40, 0, 8, 14), sample(34, 24, 40, 37, 8, 14)]
    out = run(ss, flip=[False, True, True])
    for b, s in enumerate(ss):
        assert np.array_equal(out[b].cpu().numpy(), expected(s, flip=b > 0)), b
    small = ss[1]["mask"]                                                    # no point at all: every small id becomes 0
    assert set(np.unique(out[1].cpu().numpy())) <= {0, -100} and (out[1].cpu().numpy() == 0).sum() > 0 and small.min() > 0
    assert torch.equal(run([ss[0]])[0], out[0])


@pytest.mark.parametrize("C", [2, 10, 32])
def test_class_counts(C):
    s = sample(40 + C, 24, 40, 200, 8, 14, C=C, big_rows=5)
    assert np.array_equal(run([s], C=C)[0].cpu().numpy(), expected(s, C=C))


def test_points_outside_the_image_and_labels_past_the_classes_are_counted_and_skipped():
    s = sample(50, 24, 40, 160, 8, 14, big_rows=5)
    bad = {5: ((24.5, 3.0), 1, 0.7), 40: ((-1.0, 3.0), 1, 0.7), 41: ((3.0, 40.0), 1, 0.7), 90: ((3.0, -7.5), 1, 0.7),
           91: ((float("nan"), 2.0), 1, 0.7), 120: ((6.0, 6.0), 10, 0.7), 159: ((6.0, 7.0), 255, 0.7)}
    t = {k: v.copy() for k, v in s.items()}
    for i, (pt, l, p) in bad.items():
        t["points"][i], t["labels"][i], t["probs"][i] = pt, l, p
    t["points"][7] = (-0.5, -0.25)                                           # truncates to (0, 0): inside
    keep = np.asarray([i not in bad for i in range(160)])
    clean = {"probs": t["probs"][keep], "labels": t["labels"][keep], "points": t["points"][keep], "mask": t["mask"]}
    counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    out = run([t, clean], counts=counts)
    want = expected(clean)
    assert counts.tolist() == [len(bad), 0]
    assert np.array_equal(out[0].cpu().numpy(), want) and np.array_equal(out[1].cpu().numpy(), want)


def test_more_samples_than_one_launch_takes():
    ss = [sample(60 + b % 3, 23, 37, 60 + 5 * (b % 3), 6, 20) for b in range(34)]
    want = [expected(s) for s in ss[:3]]
    out = run(ss, out=torch.empty(34, 23, 37, dtype=torch.int32, device="cuda")).cpu().numpy()
    for b in range(34):
        assert np.array_equal(out[b], want[b % 3]), b


def test_prepare_batch_returns_the_stand_alone_result_and_changes_nothing_else():
    from mopa_amd import imageprep as ip
    rng = np.random.Generator(np.random.PCG64(70))
    H, W = 40, 100
    samples, plain = [], []
    for b in range(2):
        s = sample(74 + b, H, W, 300 + 50 * b, 6, 60, big_rows=9)
        left = 31 + 2 * b
        base = {"image": dev(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)), "points_img": dev(s["points"]), "sam_mask": dev(s["mask"]),
                "crop": (left, 12, left + 50, 40), "flip": b == 1, "jitter": ((0, 2), (1.2, 0.8))}
        plain.append(base)
        samples.append({**base, "probs_2d": dev(s["probs"]), "pseudo_label_2d": dev(s["labels"]), "_np": s})
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    a = ip.prepare_batch(plain, normalizer=norm, ema_input=True)
    b = ip.prepare_batch(samples, normalizer=norm, ema_input=True)
    assert "full_2d_pslabels" not in a and set(b) == set(a) | {"full_2d_pslabels"}
    for key, va in a.items():
        vb = b[key]
        if isinstance(va, torch.Tensor):
            assert torch.equal(va, vb), key
        else:
            assert len(va) == len(vb) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(va, vb)), key
    alone = run([s["_np"] for s in samples], windows=[s["crop"] for s in samples], flip=[s["flip"] for s in samples])
    for k, s in enumerate(samples):
        got = b["full_2d_pslabels"][k]
        assert got.dtype == torch.int32 and got.shape == b["sam_mask_ls"][k].shape and torch.equal(got, alone[k])
        assert np.array_equal(got.cpu().numpy(), expected(s["_np"], window=s["crop"], flip=s["flip"]))


def test_c_abi_refuses_bad_arguments():
    from mopa_amd import _lib
    lib = _lib.load()
    s = sample(80, 24, 40, 50, 8, 14)
    t = [dev(s[k]) for k in ("probs", "labels", "points", "mask")]
    tabs = [_lib.host_ptrs([x]) for x in t]
    n = _lib.host_i32([50])
    out = torch.empty(1, 24, 40, dtype=torch.int32, device="cuda")
    need = lib.mopa_denselabels_workspace_bytes(1, 24, 40, 50, 10)
    assert need > 0 and lib.mopa_denselabels_workspace_bytes(33, 24, 40, 50, 10) == 0 and lib.mopa_denselabels_workspace_bytes(1, 24, 40, 50, 33) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def rc(B=1, C=10, oh=24, ow=40, crop=None, ws_bytes=need, n_host=n):
        return lib.mopa_denselabels(_lib.host_addr(tabs[0]), _lib.host_addr(tabs[1]), _lib.host_addr(tabs[2]), 0, _lib.host_addr(n_host),
                                    _lib.host_addr(tabs[3]), B, 24, 40, C, 96, _lib.host_addr(crop), oh, ow, None, out.data_ptr(), None,
                                    ws.data_ptr(), ws_bytes, _lib.stream())
    assert rc() == 0
    assert rc(B=0) == -1 and rc(B=33) == -1 and rc(C=1) == -1 and rc(C=33) == -1 and rc(oh=23) == -1
    assert rc(crop=_lib.host_i32([2, 0]), oh=23) == -1 and rc(crop=_lib.host_i32([0, 1]), ow=40) == -1
    assert rc(n_host=_lib.host_i32([-1])) == -1
    assert rc(ws_bytes=need - 1) == -2
    torch.cuda.synchronize()
