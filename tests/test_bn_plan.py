"""dense2d.bn_plan is the one place where a BatchNorm layer's forward and backward forms are chosen.  The specification below is the
choice as the backbone made it before there was a plan -- the forward helper, the "maxpool", "bn" and "stem" records of the backward
walk, each with its own copy of the conditions -- written out once more; the plan must equal it over every layer fact and switch
setting.  The invariants at the end were agreements between those copies.  (No GPU.)"""
import itertools

import pytest

CHANNELS = (48, 64, 128, 256, 512)
GRIDS = ((2, 80, 112), (16, 304, 480))   # stem pixels below and above STEM_BWD2_MIN_PIXELS
SWITCHES = list(itertools.product(((), ("wgrad",), ("pool",), ("wgrad", "pool")), (False, True), (False, True), (False, True)))


def spec(d, C, G, training, keep_tape, act, res, deferred, sync, biased, stem, pool_reader, grid, want_dimg):
    """-> (BnPlan, fallback).  fallback: the max-pool record left its backward to a BatchNorm record that then did not take the sums
    form and launched mopa_maxpool3x3s2_bwd itself, in front of its own backward."""
    # _backbone_forward.bn()
    if deferred:
        fwd, bits, local = "stats", False, True
    else:
        bits = bool(d.BN_MASK_BITS and keep_tape and training and res and act == 1 and C % 32 == 0 and not sync)
        if bits or (G > 1 and not (training and sync)):
            fwd, local = ("groups_bits" if bits else "groups"), True
        else:   # per group, through bn_fwd: synchronised in training mode under mopa_amd.syncbn
            fwd = "sync" if training and sync else "single"
            local = fwd != "sync"

    def second(part):   # stem_bwd2(part, B, H, W)
        return part in d.STEM_BWD2 and d.STEM_BN_FUSED_BWD and grid[0] * grid[1] * grid[2] >= d.STEM_BWD2_MIN_PIXELS
    # the "maxpool" record, which comes first in the backward walk
    pool_deferred = bool(pool_reader and second("pool") and not want_dimg and deferred)
    # the "bn" record
    stem_fused = bool(d.STEM_BN_FUSED_BWD and stem and not want_dimg and not res and act == 1 and local and C == 64)
    colsum = False
    if stem_fused:
        bwd = "sums_pool" if pool_deferred else "sums"
    else:
        fusable = local and (not res or bits)
        colsum = bool(fusable and biased and d.BN_COLSUM_FUSED)
        bwd = "fused" if fusable and (bits or colsum) else "groups" if G > 1 and local else "single" if local else "sync"
    # the "stem" record
    wgrad = "plain" if not stem_fused else "strip" if second("wgrad") else "im2col_bn"
    return d.BnPlan(fwd, bwd, bits, colsum, stem_fused and pool_deferred, wgrad), pool_deferred and not stem_fused


@pytest.mark.parametrize("stem2,stem_fused,mask_bits,colsum_fused", SWITCHES,
                         ids=lambda v: "+".join(v) or "none" if isinstance(v, tuple) else str(int(v)))
def test_bn_plan_is_what_the_backbone_chose(stem2, stem_fused, mask_bits, colsum_fused, monkeypatch):
    from mopa_amd import dense2d as d
    for name, value in (("STEM_BWD2", frozenset(stem2)), ("STEM_BN_FUSED_BWD", stem_fused), ("BN_MASK_BITS", mask_bits),
                        ("BN_COLSUM_FUSED", colsum_fused)):
        monkeypatch.setattr(d, name, value)
    flags = itertools.product(*[(False, True)] * 9)
    n = 0
    for (C, G, act, grid), (training, keep_tape, res, deferred, sync, biased, stem, pool_reader, want_dimg) in itertools.product(
            itertools.product(CHANNELS, (1, 2, 3), (0, 1), GRIDS), flags):
        if deferred and (res or act != 1):   # (BnOp.forward asserts it: a deferred layer is BatchNorm + ReLU and nothing else)
            continue
        a = (C, G, training, keep_tape, act, res, deferred, sync, biased, stem, pool_reader, grid, want_dimg)
        plan, (want, fallback) = d.bn_plan(*a), spec(d, *a)
        if fallback:
            # The one collapse: the plan never leaves a pool's backward to a layer that does not take the sums form; the max-pool record
            # launches it itself -- the same launch, at the same place in the sequence.  Only a max-pool over a deferred BatchNorm that
            # is not the stem's 64-channel bn1 got here, and the network has none.
            assert not (stem and C == 64), a
            assert not plan.pool_inside and plan == want._replace(pool_inside=False), (a, plan, want)
        else:
            assert plan == want, (a, plan, want)
        # the backward half follows what the tape holds, whatever the switch says by then
        assert d.bn_plan(*a, bits=plan.bits) == plan
        # what used to be agreements between copies
        assert not plan.bits or plan.fwd == "groups_bits", (a, plan)
        assert plan.bwd != "fused" or not res or plan.bits, (a, plan)
        if training and sync and not deferred:
            assert plan.fwd in ("sync", "single") and plan.bwd in ("sync", "single"), (a, plan)
        assert plan.pool_inside == (plan.bwd == "sums_pool"), (a, plan)
        assert (plan.stem_wgrad != "plain") == (plan.bwd in ("sums", "sums_pool")), (a, plan)
        assert not plan.colsum or plan.bwd == "fused", (a, plan)
        n += 1
    assert n == 5 * 3 * 2 * 2 * (256 + 64)   # (deferred: act and res fixed)


def test_backward_half_reads_the_bits_flag_not_the_switch(monkeypatch):
    """A residual layer whose forward pass left bits keeps the fused form when MOPA_BN_MASK_BITS is switched off before the backward
    pass, and one without bits keeps the saved-output path when it is switched on."""
    from mopa_amd import dense2d as d
    a = (64, 2, True, True, 1, True, False, False)
    monkeypatch.setattr(d, "BN_MASK_BITS", False)
    assert d.bn_plan(*a).bwd == "groups" and d.bn_plan(*a, bits=True).bwd == "fused"
    monkeypatch.setattr(d, "BN_MASK_BITS", True)
    assert d.bn_plan(*a).bwd == "fused" and d.bn_plan(*a, bits=False).bwd == "groups"
