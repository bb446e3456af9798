"""The hue step of mopa_amd/imageprep.py without a GPU: the numpy restatement of Pillow's RGB <-> HSV conversions
(tests/_hue_reference.py) equals Pillow over all 2^24 colours and all 2^24 HSV triples and reproduces fixture G14
(tests/golden_gen/g14_hue.py); draw_color_jitter draws what ColorJitter.get_params draws (restated from knowledge: torchvision is
not installed); the shift is adjust_hue's; bad arguments are refused."""
import os
import zlib

import numpy as np
import pytest
import torch

import _hue_reference as ref
from mopa_amd import imageprep as ip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_hue.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def colours():
    return ref.all_colours()


@pytest.fixture(scope="module")
def hsv_of_all_colours(colours):
    return ref.rgb_to_hsv(colours)


# ------------------------------------------------------------------------------------------------ the restatement
def test_rgb_to_hsv_equals_pillow_over_all_colours(colours, hsv_of_all_colours):
    Image = pytest.importorskip("PIL.Image")
    want = np.asarray(Image.fromarray(colours, "RGB").convert("HSV"))
    bad = np.flatnonzero((want != hsv_of_all_colours).any(-1).reshape(-1))
    assert bad.size == 0, (bad.size, colours.reshape(-1, 3)[bad[0]], want.reshape(-1, 3)[bad[0]])


def test_hsv_to_rgb_equals_pillow_over_all_triples(colours):
    """All 2^24 (H, S, V), not only those an RGB colour maps to: after the shift any H can meet any reachable (S, V)."""
    Image = pytest.importorskip("PIL.Image")
    want = np.asarray(Image.fromarray(colours, "HSV").convert("RGB"))
    got = ref.hsv_to_rgb(colours)
    bad = np.flatnonzero((want != got).any(-1).reshape(-1))
    assert bad.size == 0, (bad.size, colours.reshape(-1, 3)[bad[0]], want.reshape(-1, 3)[bad[0]])


def test_the_restatement_reproduces_the_recorded_checksums(g, hsv_of_all_colours):
    """Needs no Pillow: what Pillow gave over all colours is in the fixture."""
    for k in (2, 4):                                            # shifts 25 and 231
        hsv = hsv_of_all_colours.copy()
        hsv[..., 0] += np.uint8(g["full_shifts"][k])            # uint8 arithmetic wraps
        out = ref.hsv_to_rgb(hsv)
        assert zlib.crc32(out.tobytes()) == int(g["full_crc32"][k]) and int(out.sum(dtype=np.uint64)) == int(g["full_sum"][k])


def test_the_restatement_reproduces_the_small_cases(g):
    imgs = [g["img0"], g["img1"], g["img2"]]
    orders = set()
    for k in range(int(g["c_n"])):
        order, fs = tuple(int(o) for o in g[f"c{k}_order"]), tuple(float(f) for f in g[f"c{k}_factor"])
        orders.add(order)
        assert np.array_equal(ref.color_jitter(imgs[int(g[f"c{k}_img"])], order, fs), g[f"c{k}_out"]), (k, order, fs)
    assert len(orders) == 24 and int(g["c_n"]) == 72
    l, t, r, b = (int(v) for v in g["w_window"])
    assert np.array_equal(ref.color_jitter(imgs[0][t:b, l:r], g["w_order"], g["w_factor"]), g["w_out"])
    assert np.array_equal(np.fliplr(ref.color_jitter(imgs[1], g["f_order"], g["f_factor"])), g["f_out"])


def test_the_round_trip_is_lossy_at_shift_zero(g):
    """adjust_hue with factor 0 is not the identity, so a zero shift cannot be skipped."""
    assert not np.array_equal(ref.adjust_hue_shift(g["img0"], 0), g["img0"])


# ------------------------------------------------------------------------------------------------ the draws
def get_params(brightness, contrast, saturation, hue):
    """ColorJitter.get_params with the ranges ColorJitter.__init__ makes of its arguments."""
    fn_idx = torch.randperm(4)
    b = float(torch.empty(1).uniform_(brightness[0], brightness[1]))
    c = float(torch.empty(1).uniform_(contrast[0], contrast[1]))
    s = float(torch.empty(1).uniform_(saturation[0], saturation[1]))
    h = float(torch.empty(1).uniform_(hue[0], hue[1]))
    return fn_idx.tolist(), (b, c, s, h)


def test_draws_equal_get_params():
    for seed in range(20):
        torch.manual_seed(seed)
        order, factors = ip.draw_color_jitter(0.4, 0.4, 0.4, 0.1)
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        fn_idx, fs = get_params((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1))
        assert list(order) == fn_idx and factors == tuple(fs[op] for op in fn_idx), seed
        assert torch.equal(state, torch.get_rng_state())
        assert -0.1 <= factors[order.index(ip.HUE)] <= 0.1
    torch.manual_seed(3)
    order, factors = ip.draw_color_jitter(0.4, 0.4, 0.4, (-0.5, 0.25))
    torch.manual_seed(3)
    fn_idx, fs = get_params((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.5, 0.25))
    assert list(order) == fn_idx and factors[order.index(ip.HUE)] == fs[3]


def test_hue_off_draws_what_the_three_argument_call_draws():
    for hue in (0.0, 0, (0.0, 0.0), [0, 0]):
        torch.manual_seed(11)
        a = ip.draw_color_jitter(0.4, 0.4, 0.4)
        sa = torch.get_rng_state()
        torch.manual_seed(11)
        b = ip.draw_color_jitter(0.4, 0.4, 0.4, hue)
        assert a == b and ip.HUE not in b[0] and torch.equal(sa, torch.get_rng_state())


@pytest.mark.parametrize("hue", [-0.1, 0.6, (-0.6, 0.1), (0.2, 0.1), (0.1, 0.7), (0.1, 0.2, 0.3), "0.1", None])
def test_bad_hue_ranges_are_refused(hue):
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="hue"):
        ip.draw_color_jitter(0.4, 0.4, 0.4, hue)
    assert torch.equal(state, torch.get_rng_state())           # refused before anything is drawn


def test_the_shift_is_adjust_hues():
    for f, want in ((-0.5, 129), (-0.1, 231), (0.0, 0), (0.1, 25), (0.5, 127)):
        assert ip.hue_shift(f) == want == ref.hue_shift(f) == int(np.int32(float(np.float32(f)) * 255).astype(np.uint8)), f
    assert ip.hue_shift(-0.0039) == 0 and ip.hue_shift(0.0039) == 0 and ip.hue_shift(-0.004) == 255    # toward zero
    for f in (0.51, -0.51, float("nan")):
        with pytest.raises(ValueError):
            ip.hue_shift(f)


# ------------------------------------------------------------------------------------------------ the tables
def test_jitter_tables_carry_the_fourth_slot():
    order, factor, shift = ip._jitter_tables([((3, 1, 0, 2), (-0.1, 1.2, 0.7, 0.9)), None, ((2,), (1.1,)), ((3,), (0.5,))], 4)
    assert list(order) == [3, 1, 0, 2, -1, -1, -1, -1, 2, -1, -1, -1, 3, -1, -1, -1]
    assert list(shift) == [231, 0, 0, 127]
    assert list(factor)[:4] == [float(np.float32(v)) for v in (-0.1, 1.2, 0.7, 0.9)]
    assert ip._jitter_tables([None, ((), ())], 2) == (None, None, None)
    for bad in (((3, 3), (0.1, 0.1)), ((4,), (0.1,)), ((3,), (0.6,)), ((0, 1, 2, 3, 0), (1, 1, 1, 0, 1)), ((0,), (-0.5,))):
        with pytest.raises(ValueError):
            ip._jitter_tables([bad], 1)
