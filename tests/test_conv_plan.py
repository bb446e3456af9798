"""dense2d.conv_plan is the one place where the measured leaf rules (wino_tile, wino4_direct, wino4_conv9, wino4_fused,
wino_wgrad_eligible, wino4_wgrad_fused) are combined into what a 3x3 convolution runs as in each pass.  The specification below is
that composition written out once more, as a function of the leaf rules alone; the plan must equal it over every layer shape, batch,
map size and switch setting that the network, the tests or the profile scripts use.  (No GPU: the library is only asked the pure
size query mopa_wino4_wgrad_fused_ok.)"""
import itertools

import pytest
import torch

CHANNELS = (16, 48, 64, 96, 128, 256, 512)
PAIRS = tuple(itertools.product(CHANNELS, CHANNELS)) + ((3, 64),)
KSP = ((3, 1, 1), (3, 2, 1), (1, 1, 0))
BATCHES = (1, 2, 4, 8, 16)
MAPS = ((2, 3), (8, 12), (19, 30), (38, 60), (57, 100), (76, 120), (113, 200), (152, 240), (225, 400), (304, 480))
SETTINGS = ({}, {"WINOGRAD": False}, {"WINOGRAD_WGRAD": False}, {"F4_ROLES": ()}, {"F4_ROLES": ("dgrad", "wgrad")}, {"WINO4_DIRECT": False},
            {"WINO4_DIRECT_ROLES": ("fwd", "fwd_eval", "dgrad")}, {"WINO4_CONV9": False}, {"WINO4_WGRAD_FUSED": False},
            {"WINO4_FUSED_MIN_BLOCKS": 1 << 62}, {"WINO4_DIRECT_MIN_TILES": 0})
F4_FORMS = {3: "F4 one9", 2: "F4 one", 1: "F4 fused", 0: "F4"}


def spec_layout(d, cin, cout, B, H, W, role):
    if d.wino4_direct(cin, cout, B, H, W, role):
        return 3 if d.wino4_conv9(cin, cout, role) else 2
    return int(d.wino4_fused(cin, cout, B, H, W))


def spec(d, cin, cout, k, s, p, B, H, W, training):
    a = (cin, cout, k, s, p, B, H, W)
    Ff, Fw = d.wino_tile(*a, "fwd"), d.wino_tile(*a, "wgrad")
    Fd = d.wino_tile(cout, cin, k, s, p, B, H, W, "dgrad")
    wg = d.wino_wgrad_eligible(*a)
    one = d.wino4_wgrad_fused(cin, cout, B, H, W)
    keeps_v = bool(training and wg and Ff != 0 and Ff == Fw and not (Ff == 4 and one))
    fwd_role = "fwd" if (Ff == 4 and keeps_v) or (training and Ff != 4) else "fwd_eval"

    def conv(F, ci, co, role):
        if F != 4:
            return {0: "direct", 2: "F2"}[F], 0
        lay = spec_layout(d, ci, co, B, H, W, role)
        return F4_FORMS[lay], lay

    fwd, fwd_layout = conv(Ff, cin, cout, fwd_role)
    dgrad, dgrad_layout = conv(Fd, cout, cin, "dgrad")
    wgrad = "direct" if not wg else "F2" if Fw == 2 else "F4 one" if one else "F4"
    return d.ConvPlan(fwd=fwd, fwd_layout=fwd_layout, fwd_role=fwd_role, keeps_v=keeps_v,
                      takes_lazy=bool(Ff == 4 and (not training or (Fw == 4 and wg))),
                      wgrad=wgrad, wgrad_F={"direct": 0, "F2": 2, "F4": 4, "F4 one": 4}[wgrad], dgrad=dgrad, dgrad_layout=dgrad_layout)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()).replace(" ", "") or "defaults")
def test_conv_plan_is_the_composition_of_the_leaf_rules(setting, monkeypatch):
    from mopa_amd import dense2d as d
    for name, value in setting.items():
        monkeypatch.setattr(d, name, value)
    ops = {(cin, cout, ksp): d.ConvOp(torch.empty(cout, cin, ksp[0], ksp[0], device="meta"), None, *ksp) for cin, cout in PAIRS for ksp in KSP}
    n = 0
    for (cin, cout), (k, s, p), B, (H, W), training in itertools.product(PAIRS, KSP, BATCHES, MAPS, (False, True)):
        a = (cin, cout, k, s, p, B, H, W)
        plan, want = d.conv_plan(*a, training), spec(d, *a, training)
        assert plan == want, (a, training, plan, want)
        # the thin views
        assert d.forward_role(*a, training) == (d.wino_tile(*a, "fwd") == 4 and want.keeps_v, want.fwd_role), (a, training)
        assert ops[cin, cout, (k, s, p)].takes_lazy(B, H, W, training) == want.takes_lazy, (a, training)
        n += 1
    assert n == 50 * 3 * 5 * 10 * 2
    for (cin, cout), B, (H, W), role in itertools.product(PAIRS, BATCHES, MAPS, ("fwd", "fwd_eval", "dgrad")):
        assert d.wino4_layout(cin, cout, B, H, W, role) == spec_layout(d, cin, cout, B, H, W, role), (cin, cout, B, H, W, role)
