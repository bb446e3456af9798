"""The 2D input pipeline on the device (mopa_amd/imageprep.py, csrc/imageprep.hip) against fixture G10 -- what Pillow, scipy and the
reference's refine_sam_mask produced on the host (tests/golden_gen/g10_imageprep.py).  Every comparison is an equality.  Reads only
the committed fixtures: neither the reference checkout nor Pillow nor scipy is imported."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
NORM = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


@pytest.fixture(scope="module")
def g(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g10_imageprep.npz")))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def chw(u8):
    """uint8 (h, w, 3) -> what np.moveaxis(np.array(image, float32) / 255., -1, 0) gives."""
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(u8.astype(np.float32) / np.float32(255.0), -1, 0)))


# ---------------------------------------------------------------------------- defined identically in tests/golden_gen/g10_imageprep.py
def checksum(a) -> int:
    """Position-weighted sum of the array's bytes modulo 2^64."""
    b = np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).astype(np.uint64)
    return int((b * np.arange(1, b.size + 1, dtype=np.uint64)).sum(dtype=np.uint64))


def smooth_image(rng, H, W):
    coarse = rng.integers(0, 256, (H // 8 + 1, W // 8 + 1, 3))
    img = np.repeat(np.repeat(coarse, 8, 0), 8, 1)[:H, :W] + rng.integers(-20, 21, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def block_mask(rng, H, W, cell=32, ids=120):
    coarse = rng.integers(0, ids, (H // cell + 1, W // cell + 1))
    return np.repeat(np.repeat(coarse, cell, 0), cell, 1)[:H, :W].astype(np.uint8)


FULL = {"nuscenes": dict(W=1600, H=900, resize=(400, 225), crop=None, n=3000, seed=101),
        "a2d2": dict(W=1920, H=1208, resize=(480, 302), crop=None, n=3000, seed=102),
        "kitti": dict(W=1242, H=375, resize=None, crop=(480, 302), n=3000, seed=103)}


def fullsize_inputs(name, B=16):
    c = FULL[name]
    rng = np.random.Generator(np.random.PCG64(c["seed"]))
    H, W = c["H"], c["W"]
    out = []
    for b in range(B):
        s = {"image": smooth_image(rng, H, W), "sam_mask": block_mask(rng, H, W)}
        rows = rng.random(c["n"]) * (H * 0.6 - 1) + H * 0.4
        cols = rng.random(c["n"]) * (W - 1)
        s["points_img"] = np.stack([rows, cols], 1).astype(np.float32)
        order = ORDERS[int(rng.integers(0, 6))]
        s["jitter"] = (order, tuple(float(np.float32(rng.uniform(0.6, 1.4))) for _ in order))
        s["flip"] = bool(rng.random() < 0.5)
        if c["crop"]:
            left = int(rng.random() * (W + 1 - c["crop"][0]))
            s["crop"] = (left, H - c["crop"][1], left + c["crop"][0], H)
        out.append(s)
    return out
# ----------------------------------------------------------------------------


def on_device(samples):
    return [{k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in samples]


# ------------------------------------------------------------------------------------------------ stage by stage
def test_resize_equals_pillow(g):
    from mopa_amd import imageprep as ip
    for k in range(int(g["r_n"])):
        size = tuple(int(v) for v in g[f"r{k}_size"])
        src = dev(g[f"r{k}_in"])
        got = ip.resize_bilinear_u8([src, src.clone()], size)
        want = torch.from_numpy(g[f"r{k}_out"])
        assert got.dtype == torch.uint8 and torch.equal(got[0].cpu(), want) and torch.equal(got[1].cpu(), want), k
        # ... and through prepare_batch: only the resize and the conversion are switched on
        out = ip.prepare_batch([{"image": src, "points_img": torch.zeros(1, 2, device="cuda")}], resize=size)
        assert torch.equal(out["img"][0].cpu(), chw(g[f"r{k}_out"])), k


def test_resize_of_an_unaligned_view_and_a_preallocated_output(g):
    from mopa_amd import imageprep as ip
    src = g["r1_in"]
    size = tuple(int(v) for v in g["r1_size"])
    buf = torch.zeros(src.size + 7, dtype=torch.uint8, device="cuda")
    for off in (1, 2, 3):                                       # image bytes that start 1, 2, 3 bytes past a dword
        view = buf[off:off + src.size].view(src.shape)
        view.copy_(dev(src))
        out = torch.full((1, size[1], size[0], 3), 7, dtype=torch.uint8, device="cuda")
        ip.resize_bilinear_u8([view], size, out=out)
        assert torch.equal(out[0].cpu(), torch.from_numpy(g["r1_out"])), off


def test_jitter_equals_imageenhance(g):
    from mopa_amd import imageprep as ip
    imgs = [dev(g["j_img"][0]), dev(g["j_img"][1])]
    n = int(g["j_n"])
    cases = [(int(g[f"j{k}_img"]), tuple(int(o) for o in g[f"j{k}_order"]), tuple(float(f) for f in g[f"j{k}_factor"])) for k in range(n)]
    # all cases as ONE batch (each image with its own order and factors), then one by one through prepare_batch
    got = ip.color_jitter_u8([imgs[i] for i, _, _ in cases], [(o, f) for _, o, f in cases])
    for k, (i, order, fs) in enumerate(cases):
        assert torch.equal(got[k].cpu(), torch.from_numpy(g[f"j{k}_out"])), (k, order, fs)
    pts = torch.zeros(1, 2, device="cuda")
    out = ip.prepare_batch([{"image": imgs[i], "points_img": pts, "jitter": (o, f)} for i, o, f in cases])
    for k in range(n):
        assert torch.equal(out["img"][k].cpu(), chw(g[f"j{k}_out"])), k
    assert len({o for _, o, _ in cases if len(o) == 3}) == 6


def test_jitter_reads_through_a_crop_window(g):
    """The contrast mean is taken over the cropped image: a window equals the same call on a copy of the window."""
    from mopa_amd import imageprep as ip
    img = dev(g["j_img"][1])
    wins = [(3, 2, 36, 29), (0, 0, 33, 27), (7, 3, 40, 30)]
    jit = [((1, 0, 2), (1.4, 0.6, 0.83)), ((2, 1, 0), (1.37, 0.71, 1.23)), ((0, 1), (1.2, 0.7))]
    got = ip.color_jitter_u8([img] * 3, jit, windows=wins)
    for k, (l, t, r, b) in enumerate(wins):
        want = ip.color_jitter_u8([img[t:b, l:r].contiguous()], [jit[k]])
        assert torch.equal(got[k], want[0]), k


def test_to_tensor_equals_numpy(g):
    from mopa_amd import imageprep as ip
    src = dev(g["t_in"])
    norm = (tuple(g["t_norm"][0]), tuple(g["t_norm"][1]))
    for k in range(4):
        flip, normalise = bool(g[f"t{k}_flip"]), bool(g[f"t{k}_normalise"])
        batch = torch.zeros(3, 3, *src.shape[:2], device="cuda")
        got, ori = ip.to_tensor([src] * 3, out=batch, flip=[flip, not flip, flip], normalizer=norm if normalise else None, ori=True)
        assert got is batch
        want = torch.from_numpy(g[f"t{k}_out"])
        assert torch.equal(got[0].cpu(), want) and torch.equal(got[2].cpu(), want), k
        assert torch.equal(got[1].cpu(), torch.from_numpy(g[f"t{k ^ 1}_out"])), k
        assert torch.equal(ori[0].cpu(), torch.from_numpy(g["t0_out"])) and torch.equal(ori[1], ori[0])


def _mask_args(g, k):
    size = tuple(int(v) for v in g[f"m{k}_size"])
    window = tuple(int(v) for v in g[f"m{k}_window"])
    max_h = int(g[f"m{k}_max_h"])
    return (g[f"m{k}_in"], None if size[0] < 0 else size, None if max_h == -999999 else max_h, None if window[0] < 0 else window,
            bool(g[f"m{k}_flip"]))


def test_masks_equal_zoom_and_refine_sam_mask(g):
    from mopa_amd import imageprep as ip
    for k in range(int(g["m_n"])):
        src, size, max_h, window, flip = _mask_args(g, k)
        m = dev(src)
        got = ip.prepare_sam_mask([m, m], size=size, max_h=max_h, windows=None if window is None else [window] * 2, flip=[flip, flip])
        want = torch.from_numpy(g[f"m{k}_out"])
        assert got.dtype == torch.int32 and torch.equal(got[0].cpu(), want) and torch.equal(got[1].cpu(), want), k
        # the limit as "from these points": a point whose row is h - max_h, read by the kernel from device memory
        if max_h is not None:
            h = size[1] if size else src.shape[0]
            rm = torch.tensor([h - max_h, h - max_h], dtype=torch.int32, device="cuda")
            got = ip.prepare_sam_mask([m, m], size=size, row_min=rm, windows=None if window is None else [window] * 2, flip=[flip, flip])
            assert torch.equal(got[1].cpu(), want), k
    assert (g["m0_out"] == 5).sum() == 0 and (g["m0_out"] == 6).sum() == 55      # the threshold met exactly: removed


def test_masks_through_prepare_batch(g):
    """max_h as an int, or -- where the fixture has none -- taken from the points: a point in row 0 gives the limit 0, which cuts
    nothing."""
    from mopa_amd import imageprep as ip
    for k in range(int(g["m_n"])):
        src, size, max_h, window, flip = _mask_args(g, k)
        H, W = src.shape
        sample = {"image": torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda"), "points_img": torch.zeros(1, 2, device="cuda"),
                  "sam_mask": dev(src), "flip": flip}
        if max_h is not None:
            sample["max_h"] = max_h
        if window is not None:
            sample["crop"] = window
        out = ip.prepare_batch([sample, dict(sample)], resize=size)
        for b in range(2):
            assert torch.equal(out["sam_mask_ls"][b].cpu(), torch.from_numpy(g[f"m{k}_out"])), k


def _idx_args(g, k):
    form = str(g[f"i{k}_form"])
    if form == "resize":
        return form, dict(src_size=tuple(int(v) for v in g[f"i{k}_src_size"]), size=tuple(int(v) for v in g[f"i{k}_size"]))
    win = tuple(int(v) for v in g[f"i{k}_window"])
    return form, dict(windows=[win], size=(win[2] - win[0], win[3] - win[1]))


def test_indices_equal_the_datasets_expressions(g):
    from mopa_amd import imageprep as ip
    seen = set()
    for k in range(int(g["i_n"])):
        form, kw = _idx_args(g, k)
        p = g[f"i{k}_in"]
        seen.add((form, str(p.dtype)))
        flip = bool(g[f"i{k}_flip"])
        res = ip.prepare_img_indices([dev(p)], flip=[flip], ori=True, row_min=True, **kw)
        idx = res["img_indices"][0]
        if form == "crop":
            assert torch.equal(res["keep"][0].cpu(), torch.from_numpy(g[f"i{k}_keep"])), k
            idx = idx[res["keep"][0]]
        assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), torch.from_numpy(g[f"i{k}_out"])), k
        assert torch.equal(res["ori_img_indices"][0].cpu(), torch.from_numpy(g[f"i{k}_ori"])), k
        assert int(res["row_min"][0]) == int(g[f"i{k}_row_min"]), k
        # through prepare_batch (an all-zero image of the source size)
        W, H = (int(v) for v in g[f"i{k}_src_size"])
        sample = {"image": torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda"), "points_img": dev(p), "flip": flip}
        if form == "crop":
            sample["crop"] = kw["windows"][0]
        out = ip.prepare_batch([sample], resize=kw["size"] if form == "resize" else None, ema_input=True)
        assert torch.equal(out["img_indices"][0].cpu(), torch.from_numpy(g[f"i{k}_out"])), k
        assert torch.equal(out["ori_img_indices"][0].cpu(), torch.from_numpy(g[f"i{k}_ori"])), k
        if form == "crop":
            assert torch.equal(out["keep"][0].cpu(), torch.from_numpy(g[f"i{k}_keep"])), k
    assert seen == {(f, d) for f in ("resize", "crop") for d in ("float32", "float64")}


def test_integer_points_follow_numpys_promotion():
    """``float * floor(int array)`` is float64 in numpy and the assignment back truncates."""
    from mopa_amd import imageprep as ip
    p = np.asarray([[899, 1599], [0, 0], [450, 801], [7, 13]], np.int32)
    q = p.copy()
    q[:, 0] = float(225) / 900 * np.floor(q[:, 0])
    q[:, 1] = float(400) / 1600 * np.floor(q[:, 1])
    res = ip.prepare_img_indices([dev(p)], src_size=(1600, 900), size=(400, 225))
    assert torch.equal(res["img_indices"][0].cpu(), torch.from_numpy(q.astype(np.int64)))


# ------------------------------------------------------------------------------------------------ the whole pipeline
def _p_samples(g):
    return [{"image": dev(g[f"p{b}_image"]), "sam_mask": dev(g[f"p{b}_sam_mask"]), "points_img": dev(g[f"p{b}_points"]),
             "jitter": (tuple(int(o) for o in g[f"p{b}_order"]), tuple(float(f) for f in g[f"p{b}_factor"])),
             "flip": bool(g[f"p{b}_flip"])} for b in range(2)]


def _p_run(g):
    from mopa_amd import imageprep as ip
    norm = (tuple(g["p_norm"][0]), tuple(g["p_norm"][1]))
    return ip.prepare_batch(_p_samples(g), resize=tuple(int(v) for v in g["p_size"]), normalizer=norm, ema_input=True)


def test_prepare_batch_equals_the_reference_pipeline(g):
    out = _p_run(g)
    assert out["img"].shape == (2, 3, 40, 56) and out["img"].dtype == torch.float32
    for b in range(2):
        assert torch.equal(out["img"][b].cpu(), torch.from_numpy(g[f"p{b}_img"])), b
        assert torch.equal(out["ori_img"][b].cpu(), torch.from_numpy(g[f"p{b}_ori_img"])), b
        assert torch.equal(out["sam_mask_ls"][b].cpu(), torch.from_numpy(g[f"p{b}_mask"])), b
        assert torch.equal(out["img_indices"][b].cpu(), torch.from_numpy(g[f"p{b}_idx"])), b
        assert torch.equal(out["ori_img_indices"][b].cpu(), torch.from_numpy(g[f"p{b}_ori_idx"])), b


def _loss_bits(img, img_indices, masks):
    from mopa_amd.common.utils.loss import mask_cons_loss, softmax_lastdim
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d
    torch.manual_seed(0)
    model = build_model_2d(default_cfg())[0].cuda().train()
    model.net_2d.dropout.p = 0.0
    o = model({"img": img, "img_indices": img_indices})
    loss = o["seg_logit"].square().mean() + 0.01 * mask_cons_loss(softmax_lastdim(o["seg_logit_all"]), masks, True)
    loss.backward()
    grads = torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])
    return loss.detach().clone(), grads.clone()


def test_prepare_batch_feeds_net2dseg_and_mask_cons_loss_unchanged(g):
    """Forward + backward of Net2DSeg and mask_cons_loss on prepare_batch's output, with no conversion in between, gives the bits
    that the fixture's arrays give when they are uploaded as a loader would hand them over."""
    out = _p_run(g)
    loss_a, grads_a = _loss_bits(out["img"], out["img_indices"], out["sam_mask_ls"])
    img = torch.stack([torch.from_numpy(g[f"p{b}_img"]) for b in range(2)]).cuda()
    loss_b, grads_b = _loss_bits(img, [g[f"p{b}_idx"] for b in range(2)], [torch.from_numpy(g[f"p{b}_mask"]) for b in range(2)])
    assert torch.isfinite(loss_a) and torch.equal(loss_a, loss_b) and torch.equal(grads_a, grads_b)


# ------------------------------------------------------------------------------------------------ full size
def _run_full(name):
    from mopa_amd import imageprep as ip
    samples = on_device(fullsize_inputs(name))
    return ip.prepare_batch(samples, resize=FULL[name]["resize"], normalizer=NORM, ema_input=True)


@pytest.mark.parametrize("name", ["nuscenes", "a2d2", "kitti"])
def test_full_size_batches_equal_the_recorded_checksums(name, golden_dir):
    """B = 8 + 8 samples of the real shapes; every output against the checksum recorded from the host calls."""
    with open(os.path.join(golden_dir, "g10_imageprep_fullsize.json")) as f:
        want = json.load(f)[name]
    out = _run_full(name)
    c = FULL[name]
    w, h = c["resize"] or c["crop"]
    assert out["img"].shape == (16, 3, h, w)
    assert checksum(out["img"].cpu().numpy()) == want["img"]
    assert checksum(torch.stack(out["ori_img"]).cpu().numpy()) == want["ori_img"]
    masks = torch.stack(out["sam_mask_ls"]).cpu().numpy()
    assert int((masks == -100).sum()) == want["n_ignored"] and checksum(masks) == want["sam_mask"]
    idx = torch.cat(out["img_indices"]).cpu().numpy()
    assert len(idx) == want["n_indices"] and checksum(idx) == want["img_indices"]
    assert checksum(torch.cat(out["ori_img_indices"]).cpu().numpy()) == want["ori_img_indices"]
    if "keep" in want:
        assert checksum(torch.cat(out["keep"]).cpu().numpy().astype(np.uint8)) == want["keep"]
    # two runs give identical bits
    again = _run_full(name)
    assert torch.equal(out["img"], again["img"])
    for key in ("ori_img", "sam_mask_ls", "img_indices", "ori_img_indices"):
        assert all(torch.equal(a, b) for a, b in zip(out[key], again[key])), key


def test_more_images_than_one_launch_takes(g):
    """40 images: the binding splits the batch into launches of at most 32."""
    from mopa_amd import imageprep as ip
    src = dev(g["r1_in"])
    size = tuple(int(v) for v in g["r1_size"])
    jit = [(ORDERS[b % 6], (0.9, 1.2, 0.7)) for b in range(40)]
    out = ip.prepare_batch([{"image": src, "points_img": torch.zeros(1, 2, device="cuda"), "jitter": jit[b], "flip": b % 2 == 1}
                            for b in range(40)], resize=size)
    for b in range(40):
        assert torch.equal(out["img"][b], out["img"][b % 12]), b        # orders repeat with period 6, flips with period 2


def test_no_host_sync_in_the_resize_form(g):
    """nuScenes / A2D2 form with resident inputs: nothing synchronises, tables included (they are uploaded through pinned
    memory).  The crop form (SemanticKITTI) compacts the index arrays by the keep mask, which takes ONE read-back per call, as
    voxelize_scan does; it is not run under this mode."""
    samples = _p_samples(g)
    out_t = torch.empty(2, 3, 40, 56, device="cuda")
    _p_run(g)                                                   # allocator warm-up; the tables stay cached
    from mopa_amd import imageprep as ip
    ip._tables.clear()                                          # ... so drop them: their upload must not synchronise either
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ip.prepare_batch(samples, out=out_t, resize=(56, 40), normalizer=NORM, ema_input=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.cuda.get_sync_debug_mode() == prev and out["img"] is out_t
    for b in range(2):
        assert torch.equal(out["img"][b].cpu(), torch.from_numpy(g[f"p{b}_img"]))
        assert torch.equal(out["sam_mask_ls"][b].cpu(), torch.from_numpy(g[f"p{b}_mask"]))


def test_c_abi_refuses_bad_arguments():
    from mopa_amd._lib import call
    with pytest.raises(RuntimeError):
        call("mopa_imageprep_resize_u8", None, 1, 8, 8, None, 3, None, 3, 4, 4, 8, None, 0)
    with pytest.raises(RuntimeError):
        call("mopa_imageprep_pixels", None, 33, 24, 8, 8, None, None, None, None, None, None, None, None, 0)
