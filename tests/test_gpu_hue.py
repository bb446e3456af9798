"""Operation 3 of the colour jitter on the device (mopa_amd/imageprep.py, csrc/imageprep.hip: ip_hue) against fixture G14 -- what
Pillow's HSV round trip behind torchvision's adjust_hue, alone and between ImageEnhance's blends, produced on the host
(tests/golden_gen/g14_hue.py) -- and against the numpy restatement the generator held against Pillow (tests/_hue_reference.py).
Every comparison is an equality.  Reads only the committed fixtures: Pillow is not imported."""
import ctypes
import itertools
import os
import zlib

import numpy as np
import pytest
import torch

import _hue_reference as ref

pytestmark = pytest.mark.gpu

SHIFTS = (0, 1, 25, 128, 231, 255)


@pytest.fixture(scope="module")
def g(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g14_hue.npz")))


@pytest.fixture(scope="module")
def g10(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g10_imageprep.npz")))


@pytest.fixture(scope="module")
def colours():
    return dev(ref.all_colours())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def chw(u8):
    """uint8 (h, w, 3) -> what np.moveaxis(np.array(image, float32) / 255., -1, 0) gives."""
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(u8.astype(np.float32) / np.float32(255.0), -1, 0)))


def case(g, k):
    return int(g[f"c{k}_img"]), tuple(int(o) for o in g[f"c{k}_order"]), tuple(float(f) for f in g[f"c{k}_factor"])


def factor_of(shift):
    """A hue factor whose shift is `shift`; 128 has none (factors in [-0.5, 0.5] reach 0..127 and 129..255)."""
    f = (shift + 0.5) / 255 if shift < 128 else -(256 - shift + 0.5) / 255
    from mopa_amd import imageprep as ip
    assert ip.hue_shift(f) == shift
    return f


# ------------------------------------------------------------------------------------------------ the C ABI, called directly
def raw(imgs, orders, factors, shifts, slots, out, sums):
    """mopa_imageprep_contrast_sums[4] + mopa_imageprep_pixels[4] on B images (H, W, 3) with the host arrays as given."""
    from mopa_amd._lib import call, host_addr, host_i32, host_ptrs, ptr, stream
    B, (H, W, _) = len(imgs), imgs[0].shape
    tab = host_ptrs(imgs)
    o = host_i32([v for row in orders for v in row])
    f = (ctypes.c_float * (slots * B))(*[v for row in factors for v in row])
    sh = None if shifts is None else host_i32(shifts)
    extra = (host_addr(sh),) if slots == 4 else ()
    sfx = "4" if slots == 4 else ""
    call("mopa_imageprep_contrast_sums" + sfx, host_addr(tab), B, W * 3, H, W, host_addr(o), host_addr(f), *extra, ptr(sums), stream())
    call("mopa_imageprep_pixels" + sfx, host_addr(tab), B, W * 3, H, W, host_addr(o), host_addr(f), *extra, ptr(sums), None, ptr(out),
         None, None, None, stream())


# ------------------------------------------------------------------------------------------------ all 2^24 colours
@pytest.mark.parametrize("shift", SHIFTS)
def test_all_colours_equal_pillow(g, colours, shift):
    """Hue only on the 4096 x 4096 image of every colour: CRC32 and byte sum of what Pillow gave.  Shift 128 belongs to no factor
    of the public range and goes through the entry point."""
    from mopa_amd import imageprep as ip
    k = list(g["full_shifts"]).index(shift)
    if shift == 128:
        out = torch.empty(1, 4096, 4096, 3, dtype=torch.uint8, device="cuda")
        raw([colours], [(3, -1, -1, -1)], [(1.0,) * 4], [shift], 4, out, torch.zeros(1, dtype=torch.int64, device="cuda"))
    else:
        out = ip.color_jitter_u8([colours], [((3,), (factor_of(shift),))])
    got = out[0].cpu().numpy()
    if zlib.crc32(got.tobytes()) != int(g["full_crc32"][k]) or int(got.sum(dtype=np.uint64)) != int(g["full_sum"][k]):
        want = ref.adjust_hue_shift(ref.all_colours(), shift).reshape(-1, 3)
        bad = np.flatnonzero((want != got.reshape(-1, 3)).any(-1))
        n = int(bad[0]) if bad.size else -1
        pytest.fail(f"shift {shift}: {bad.size} colours differ; the first is {(n >> 16, (n >> 8) & 255, n & 255)}: "
                    f"{got.reshape(-1, 3)[n]} for {want[n]}")


# ------------------------------------------------------------------------------------------------ the small cases
def test_all_orders_equal_pillow_as_one_batch(g):
    from mopa_amd import imageprep as ip
    imgs = [dev(g[f"img{i}"]) for i in range(3)]
    cases = [case(g, k) for k in range(int(g["c_n"]))]
    assert len({o for _, o, _ in cases}) == 24
    for i in range(3):                                          # one size per call: the 24 orders of an image are one batch
        ks = [k for k, c in enumerate(cases) if c[0] == i]
        got = ip.color_jitter_u8([imgs[i]] * len(ks), [cases[k][1:] for k in ks])
        for n, k in enumerate(ks):
            assert torch.equal(got[n].cpu(), torch.from_numpy(g[f"c{k}_out"])), (k,) + cases[k]


def test_all_orders_equal_pillow_one_by_one_through_prepare_batch(g):
    """B = 1 per call; in the orders with hue in front of contrast the mean must be the shifted image's."""
    from mopa_amd import imageprep as ip
    imgs = [dev(g[f"img{i}"]) for i in range(3)]
    pts = torch.zeros(1, 2, device="cuda")
    for k in range(int(g["c_n"])):
        i, order, fs = case(g, k)
        out = ip.prepare_batch([{"image": imgs[i], "points_img": pts, "jitter": (order, fs)}])
        assert torch.equal(out["img"][0].cpu(), chw(g[f"c{k}_out"])), (k, i, order, fs)


def test_hue_reads_through_a_crop_window(g):
    from mopa_amd import imageprep as ip
    img = dev(g["img0"])
    win = tuple(int(v) for v in g["w_window"])
    jit = (tuple(int(o) for o in g["w_order"]), tuple(float(f) for f in g["w_factor"]))
    assert jit[0].index(3) < jit[0].index(1)
    got = ip.color_jitter_u8([img, img], [jit, jit], windows=[win, win])
    assert torch.equal(got[0].cpu(), torch.from_numpy(g["w_out"])) and torch.equal(got[1], got[0])
    out = ip.prepare_batch([{"image": img, "points_img": torch.tensor([[10.0, 20.0]], device="cuda"), "jitter": jit, "crop": win}])
    assert torch.equal(out["img"][0].cpu(), chw(g["w_out"]))


def test_hue_and_flip(g):
    from mopa_amd import imageprep as ip
    jit = (tuple(int(o) for o in g["f_order"]), tuple(float(f) for f in g["f_factor"]))
    out = ip.prepare_batch([{"image": dev(g["img1"]), "points_img": torch.zeros(1, 2, device="cuda"), "jitter": jit, "flip": True}])
    assert torch.equal(out["img"][0].cpu(), chw(g["f_out"]))


@pytest.mark.parametrize("w", [1, 3, 255, 256, 257])
def test_widths_around_the_row_segment(w):
    """256 pixels of a row are one block's segment: one short of it, exactly it, one more; with and without flip, as uint8 and as
    the float batch tensor; hue in front of contrast."""
    from mopa_amd import imageprep as ip
    rng = np.random.Generator(np.random.PCG64(1400 + w))
    img = rng.integers(0, 256, (3, w, 3)).astype(np.uint8)
    jit = ((3, 1, 2, 0), (-0.23, 1.3, 0.6, 0.9))
    want = ref.color_jitter(img, *jit)
    d = dev(img)
    assert torch.equal(ip.color_jitter_u8([d], [jit])[0].cpu(), torch.from_numpy(want))
    got = ip.to_tensor([d, d], flip=[False, True], jitter=[jit, jit])
    assert torch.equal(got[0].cpu(), chw(want)) and torch.equal(got[1].cpu(), chw(np.fliplr(want)))


def test_a_batch_of_33_images():
    """One more than a launch takes: the binding splits, and every image keeps its own order, factors and shift."""
    from mopa_amd import imageprep as ip
    rng = np.random.Generator(np.random.PCG64(1433))
    orders = list(itertools.permutations(range(4)))
    imgs = [rng.integers(0, 256, (6, 10, 3)).astype(np.uint8) for _ in range(33)]
    jit = []
    for b in range(33):
        order = orders[(7 * b) % 24][:1 + b % 4]
        jit.append((order, tuple(float(np.float32(rng.uniform(-0.5, 0.5) if op == 3 else rng.uniform(0.6, 1.4))) for op in order)))
    jit[5] = None
    jit[32] = ((3, 1), (-0.3, 1.2))                             # the image of the second launch has a shift of its own
    got = ip.color_jitter_u8([dev(im) for im in imgs], jit)
    for b in range(33):
        want = imgs[b] if jit[b] is None else ref.color_jitter(imgs[b], *jit[b])
        assert torch.equal(got[b].cpu(), torch.from_numpy(want)), (b, jit[b])


# ------------------------------------------------------------------------------------------------ old and new entry points
def test_hue_free_jitter_is_the_same_through_both_entry_points(g10):
    """G10's jitter cases through the three-slot entry points and, with a fourth slot of -1, through the four-slot ones: the same
    sums and the same bytes (and those of the fixture)."""
    n = int(g10["j_n"])
    imgs = [dev(g10["j_img"][0]), dev(g10["j_img"][1])]
    cases = [(int(g10[f"j{k}_img"]), [int(o) for o in g10[f"j{k}_order"]], [float(f) for f in g10[f"j{k}_factor"]]) for k in range(n)]
    H, W, _ = imgs[0].shape
    res = {}
    for slots in (3, 4):
        outs, sums = [], []
        for s in range(0, n, 32):
            part = cases[s:s + 32]
            out = torch.empty(len(part), H, W, 3, dtype=torch.uint8, device="cuda")
            sm = torch.zeros(len(part), dtype=torch.int64, device="cuda")
            raw([imgs[i] for i, _, _ in part], [o + [-1] * (slots - len(o)) for _, o, _ in part],
                [f + [1.0] * (slots - len(f)) for _, _, f in part], [0] * len(part) if slots == 4 else None, slots, out, sm)
            outs.append(out)
            sums.append(sm)
        res[slots] = (torch.cat(outs), torch.cat(sums))
    assert torch.equal(res[3][0], res[4][0]) and torch.equal(res[3][1], res[4][1])
    for k in range(n):
        assert torch.equal(res[4][0][k].cpu(), torch.from_numpy(g10[f"j{k}_out"])), k


REFUSED = [("hue twice", 4, [(3, 3, -1, -1)], [7]),
           ("a gap", 4, [(3, -1, 0, -1)], [7]),
           ("shift 256", 4, [(3, 0, -1, -1)], [256]),
           ("shift -1", 4, [(0, 3, -1, -1)], [-1]),
           ("operation 4", 4, [(4, -1, -1, -1)], [7]),
           ("hue through the three-slot entry points", 3, [(3, -1, -1)], None),
           ("hue through the three-slot entry points, last", 3, [(0, 1, 3)], None)]


@pytest.mark.parametrize("what,slots,orders,shifts", REFUSED, ids=[r[0] for r in REFUSED])
def test_c_abi_refusals_write_nothing(what, slots, orders, shifts):
    """Every check comes before the first launch (and before the sums are zeroed): the outputs keep their sentinel.  The second
    image of the call is the bad one, so the first one's slots have been accepted when the call is refused."""
    from mopa_amd._lib import call, host_addr, host_i32, host_ptrs, ptr, stream
    img = torch.full((4, 5, 3), 90, dtype=torch.uint8, device="cuda")
    good = (0, 1, 2, -1)[:slots]
    o = host_i32(list(good) + list(orders[0]))
    f = (ctypes.c_float * (2 * slots))(*([0.9] * (2 * slots)))
    sh = None if shifts is None else host_i32([3] + shifts)
    extra = (host_addr(sh),) if slots == 4 else ()
    sfx = "4" if slots == 4 else ""
    tab = host_ptrs([img, img])
    out = torch.full((2, 4, 5, 3), 171, dtype=torch.uint8, device="cuda")
    out_f = torch.full((2, 3, 4, 5), -7.0, device="cuda")
    sums = torch.full((2,), 12345, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        call("mopa_imageprep_contrast_sums" + sfx, host_addr(tab), 2, 15, 4, 5, host_addr(o), host_addr(f), *extra, ptr(sums), stream())
    with pytest.raises(RuntimeError):
        call("mopa_imageprep_pixels" + sfx, host_addr(tab), 2, 15, 4, 5, host_addr(o), host_addr(f), *extra, ptr(sums), None,
             ptr(out), ptr(out_f), None, None, stream())
    torch.cuda.synchronize()
    assert bool((out == 171).all()) and bool((out_f == -7.0).all()) and bool((sums == 12345).all()), what


def test_the_same_call_is_accepted_once_mended():
    """The refusal test's call with a legal second image runs: its refusals are of the bad slot, not of the call's shape."""
    img = torch.full((4, 5, 3), 90, dtype=torch.uint8, device="cuda")
    img[1, 2] = torch.tensor([200, 30, 90], dtype=torch.uint8)
    out = torch.full((2, 4, 5, 3), 171, dtype=torch.uint8, device="cuda")
    sums = torch.full((2,), 12345, dtype=torch.int64, device="cuda")
    raw([img, img], [(0, 1, 2, -1), (3, 0, -1, -1)], [(0.9,) * 4] * 2, [3, 255], 4, out, sums)
    im = img.cpu().numpy()
    assert torch.equal(out[0].cpu(), torch.from_numpy(ref.color_jitter(im, (0, 1, 2), (0.9, 0.9, 0.9))))
    assert torch.equal(out[1].cpu(), torch.from_numpy(ref._blend(np.zeros_like(im), ref.adjust_hue_shift(im, 255), 0.9)))
