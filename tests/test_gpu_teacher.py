"""mopa_amd.teacher on the device: the EMA weights in place, the student untouched, the replayed eval forward, no stale weight
forms, live BatchNorm buffers, batching, pseudo labels and the host-synchronisation contract; plus the device index packer.

Shapes are the smallest that still take every path: 64 x 96 images (a multiple of 16) and 48 x 80 / 45 x 80 (padded), about 2,000
points per scan, two images per batch (one pass of two, or two passes of one)."""
import os

import numpy as np
import pytest
import torch

from oracle.params import det_tensor

pytestmark = pytest.mark.gpu

H, W, NPTS, C = 64, 96, 2000, 5


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_batch(seed, sizes=((H, W), (H, W)), n=NPTS, device_indices=True):
    rng = np.random.Generator(np.random.PCG64(seed))
    imgs = [torch.from_numpy(rng.random((3, h, w), dtype=np.float32)).cuda() for h, w in sizes]
    idx = [np.stack([rng.integers(0, h, n + 13 * b), rng.integers(0, w, n + 13 * b)], 1).astype(np.int64) for b, (h, w) in enumerate(sizes)]
    locs = np.concatenate([np.concatenate([rng.integers(0, 400, (len(ix), 2)), rng.integers(0, 40, (len(ix), 1)),
                                           np.full((len(ix), 1), b)], 1) for b, ix in enumerate(idx)]).astype(np.int64)
    batch = {"img": torch.stack(imgs) if len(set(sizes)) == 1 else imgs,
             "img_indices": [cu(i) for i in idx] if device_indices else idx,
             "x": [cu(locs), torch.ones(len(locs), 1, device="cuda")]}
    label = cu(rng.integers(0, C, len(locs)).astype(np.int64))
    return batch, label


class World:
    """Both networks with dropout off, FlatAdam + FlatEMA (decay 0.5) each, after two optimizer steps and two EMA updates:
    shadow != live != init."""

    def __init__(self, steps=2):
        from mopa_amd.config import default_cfg
        from mopa_amd.models.build import build_model_2d, build_model_3d
        from mopa_amd.optim import FlatAdam
        from mopa_amd.pseudo import FlatEMA
        torch.manual_seed(0)
        cfg = default_cfg(C, True)
        self.m2, self.m3 = build_model_2d(cfg)[0].cuda().train(), build_model_3d(cfg)[0].cuda().train()
        self.m2.net_2d.dropout.p = 0.0
        self.o2, self.o3 = FlatAdam(self.m2.parameters(), lr=1e-3), FlatAdam(self.m3.parameters(), lr=1e-3)
        self.e2, self.e3 = FlatEMA(self.o2, 0.5, use_num_updates=False), FlatEMA(self.o3, 0.5, use_num_updates=False)
        self.batch, self.label = make_batch(1)
        for _ in range(steps):
            self.step()
            self.e2.update()
            self.e3.update()

    def step(self):
        from mopa_amd.common.utils.loss import seg_ce
        self.o2.zero_grad()
        self.o3.zero_grad()
        o2, o3 = self.m2(self.batch), self.m3(self.batch)
        l2 = seg_ce(o2["seg_logit"], self.label) + seg_ce(o2["seg_logit2"], self.label)
        l3 = seg_ce(o3["seg_logit"], self.label) + seg_ce(o3["seg_logit2"], self.label)
        l2.backward()
        l3.backward()
        g2, g3 = self.o2.grad.clone(), self.o3.grad.clone()
        self.o2.step()
        self.o3.step()
        return l2.detach().clone(), l3.detach().clone(), g2, g3

    def teacher(self, **kw):
        from mopa_amd.teacher import Teacher
        return Teacher(self.m2, self.m3, self.e2, self.e3, **kw)


def eval_per_image(m2, m3, batch):
    """One eval call per image and one 3D call, as the reference's loop makes them -> the Teacher's keys."""
    imgs = batch["img"]
    outs = [m2({"img": imgs[i][None] if imgs[i].dim() == 3 else imgs[i:i + 1], "img_indices": [batch["img_indices"][i]]})
            for i in range(len(imgs))]
    o3 = m3({"x": batch["x"]})
    return {"seg_logit_2d": torch.cat([o["seg_logit"] for o in outs]), "seg_logit2_2d": torch.cat([o["seg_logit2"] for o in outs]),
            "seg_logit_all": torch.cat([o["seg_logit_all"] for o in outs]), "seg_logit_3d": o3["seg_logit"], "seg_logit2_3d": o3["seg_logit2"]}


def by_hand(w, batch):
    """INTEGRATION.md's recipe before this module: average_parameters(), model.eval(), one call per image."""
    with torch.no_grad():
        with w.e2.average_parameters(), w.e3.average_parameters():
            w.m2.eval()
            w.m3.eval()
            out = eval_per_image(w.m2, w.m3, batch)
    w.m2.train()
    w.m3.train()
    return out


def assert_same(a, b, keys=None):
    for k in keys or b.keys():
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 1. packer
def test_pack_point_pix_equals_pack_indices():
    from mopa_amd.models.xmuda_arch import Net2DSeg
    from mopa_amd.teacher import pack_point_pix
    h, w = 45, 80   # padded to 48 x 80
    rng = np.random.Generator(np.random.PCG64(7))
    idx = [np.stack([rng.integers(0, h, n), rng.integers(0, w, n)], 1).astype(np.int64) for n in (700, 0, 331)]
    idx[0][0], idx[2][-1] = (0, 0), (h - 1, w - 1)
    ref = Net2DSeg.pack_indices(idx, h, w, "cuda")
    pix, status = pack_point_pix([cu(i) for i in idx], h, w, torch.device("cuda"))
    assert pix.dtype == torch.int32 and torch.equal(pix, ref) and int(status) == 0
    assert int(pix[0]) == 0 and int(pix[-1]) == (2 * 48 + h - 1) * 80 + w - 1
    # three indices out of range: counted, and clamped into their own image
    bad = [i.copy() for i in idx]
    bad[0][5], bad[0][6], bad[2][7] = (-1, 3), (h, 3), (2, w + 100)
    pix, status = pack_point_pix([cu(i) for i in bad], h, w, torch.device("cuda"))
    assert int(status) == 3
    clamped = [i.copy() for i in idx]
    clamped[0][5], clamped[0][6], clamped[2][7] = (0, 3), (h - 1, 3), (2, w - 1)
    assert torch.equal(pix, Net2DSeg.pack_indices(clamped, h, w, "cuda"))
    with pytest.raises(IndexError):
        Net2DSeg.pack_indices(bad, h, w, "cuda")


def test_predict_raises_on_bad_device_indices_when_validating(monkeypatch):
    w = World(steps=0)
    batch, _ = make_batch(3, n=50)
    batch["img_indices"][1][4, 1] = W
    t = w.teacher()
    t.predict(batch)     # unchecked by default: the index is clamped, its count stays on the device
    assert t.last_index_status.shape == (1,) and int(t.last_index_status) == 1
    monkeypatch.setenv("MOPA_VALIDATE_LABELS", "1")
    with pytest.raises(IndexError):
        t.predict(batch)


# ------------------------------------------------------------------------------------------------ 2. shadow weights in place
def test_shadow_weights_in_place_equal_the_by_hand_recipe():
    w = World()
    assert not torch.equal(w.e2.shadow, w.o2.flat) and not torch.equal(w.e3.shadow, w.o3.flat)
    ref = by_hand(w, w.batch)
    out = w.teacher().predict(w.batch, batched=False, heads="all")
    assert set(out) == set(ref)
    assert_same(out, ref)
    assert all(v.dtype == torch.float32 for v in out.values())


# ------------------------------------------------------------------------------------------------ 3. student untouched
def student_state(w):
    from mopa_amd._lib import WEIGHTS_EPOCH
    bufs = {f"{i}.{k}": v.clone() for i, m in enumerate((w.m2, w.m3)) for k, v in m.named_buffers()}
    return {"flat2": w.o2.flat.clone(), "flat3": w.o3.flat.clone(), "epoch": WEIGHTS_EPOCH[0], "bufs": bufs, "calls": w.m2._calls,
            "training": (w.m2.training, w.m3.training, w.m2.net_2d.training, w.m3.net_3d.training),
            "shadow2": w.e2.shadow.clone(), "shadow3": w.e3.shadow.clone()}


def student_caches(w):
    """Keys, validity tags and tensor identities of the student's derived weight forms, its recorded 2D lists and its native 3D
    executor state: a teacher that read, refreshed or replaced one of them would change this."""
    from mopa_amd import dense2d, sparse3d
    graphs = w.m2._cache.__dict__.get("graphs2d", {})
    nat = w.m3._cache.__dict__.get("native")
    return {"forms2d": {k: (v[0], id(v[1]), v[1]._version) for k, v in dense2d._relayout_cache.items()},
            "forms3d": {k: (v[0], id(v[1]), v[1]._version) for k, v in sparse3d._weight_cache.items()},
            "refreshed": (dict(dense2d._refreshed), dict(sparse3d._refreshed)),
            "graphs2d": {k: (id(g), g.calls, id(g.fwd), id(g.bwd), g.failed, g.generation) for k, g in graphs.items()},
            "native": None if nat is None else (id(nat), nat.epoch, nat._tag, nat.params.tobytes(), nat.forms.tobytes(), nat.grads.tobytes()),
            "cache_flat": id(w.m2._cache.flat), "cache_flat3": id(w.m3._cache.flat)}


def test_student_untouched_and_next_step_equals_the_twin_run():
    a, b = World(), World()
    assert torch.equal(a.o2.flat, b.o2.flat) and torch.equal(a.o3.flat, b.o3.flat)   # the twin runs agree before the teacher is called
    before, caches = student_state(a), student_caches(a)
    assert caches["forms2d"] and caches["graphs2d"] and caches["native"] is not None    # (the two training steps left them behind)
    t = a.teacher()
    for _ in range(3):   # eager, recorded, replayed
        t.predict(a.batch)
        t.pseudo_labels(dict(a.batch, gather=torch.arange(len(a.label), device="cuda")), xm=True)
    after = student_state(a)
    assert t.stats["replays"] >= 2
    assert student_caches(a) == caches
    assert any("num_batches_tracked" in k for k in before["bufs"])
    for k in ("epoch", "calls", "training"):
        assert before[k] == after[k], k
    for k in ("flat2", "flat3", "shadow2", "shadow3"):
        assert torch.equal(before[k], after[k]), k
    for k, v in before["bufs"].items():
        assert torch.equal(v, after["bufs"][k]), k
    ra, rb = a.step(), b.step()
    for x, y in zip(ra, rb):    # losses and gradients
        assert torch.equal(x, y)
    assert torch.equal(a.o2.flat, b.o2.flat) and torch.equal(a.o3.flat, b.o3.flat)
    for (k, x), (_, y) in zip(list(a.m2.named_buffers()) + list(a.m3.named_buffers()), list(b.m2.named_buffers()) + list(b.m3.named_buffers())):
        assert torch.equal(x, y), k


# ------------------------------------------------------------------------------------------------ 4. replay
def test_replayed_eval_forward():
    w = World()
    t, plain = w.teacher(), w.teacher(replay=False)
    outs = [t.predict(w.batch, heads="all") for _ in range(3)]
    assert t.stats["replays"] >= 1 and t.stats["recorded"] == 1 and t.stats["failed"] == 0
    ref = plain.predict(w.batch, heads="all")
    assert plain.stats["replays"] == 0 and not plain.graphs
    for o in outs:
        assert_same(o, ref)
    # a second shape gets its own key
    small, _ = make_batch(5, sizes=((48, 80), (48, 80)))
    souts = [t.predict(small) for _ in range(3)]
    assert len(t.graphs) == 2 and t.stats["recorded"] == 2
    sref = plain.predict(small)
    for o in souts:
        assert_same(o, sref)
    assert_same(t.predict(w.batch, heads="all"), ref)    # the first key still replays the right pass
    # a list with both sizes comes back in input order
    mixed, _ = make_batch(6, sizes=((48, 80), (H, W), (48, 80)), n=500)
    got = t.predict(mixed, heads="all")
    one = plain.predict(mixed, batched=False, heads="all")
    ns = [len(i) for i in mixed["img_indices"]]
    for k in ("seg_logit_2d", "seg_logit2_2d"):
        assert got[k].shape == one[k].shape
        # (the two 48 x 80 images share a pass here and have one each there: the parity bound of the G1 fixtures, not bit identity)
        np.testing.assert_allclose(got[k].cpu().numpy(), one[k].cpu().numpy(), rtol=1e-3, atol=2e-4)
    assert [tuple(x.shape[:2]) for x in got["seg_logit_all"]] == [(48, 80), (H, W), (48, 80)]
    # the middle image is a pass of its own either way: bit-identical, at its place
    assert torch.equal(got["seg_logit_2d"].split(ns)[1], one["seg_logit_2d"].split(ns)[1])
    assert torch.equal(got["seg_logit_all"][1], one["seg_logit_all"][1])
    assert torch.equal(got["seg_logit_3d"], one["seg_logit_3d"])


def test_a_failed_recording_keeps_the_key_eager(monkeypatch):
    from mopa_amd import dense2d
    w = World()
    ref = w.teacher(replay=False).predict(w.batch, heads="all")
    attempts = []

    def refuse(self, P, flat):
        attempts.append(1)
        raise RuntimeError("CommandList: an entry point takes a host pointer of unknown size and cannot be recorded")
    monkeypatch.setattr(dense2d.Graph2D, "record_eval", refuse)
    t = w.teacher()
    for _ in range(4):
        assert_same(t.predict(w.batch, heads="all"), ref)
    (g,) = t.graphs.values()
    assert g.failed and g.fwd is None and len(attempts) == 1      # tried once, eager for good
    assert t.stats == {"replays": 0, "recorded": 0, "eager": 4, "dropped": 0, "failed": 1}


# ------------------------------------------------------------------------------------------------ 5. no stale forms
def fresh_pair(w):
    """A new model pair: parameters from the EMA state dict, buffers from the live models."""
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d, build_model_3d
    cfg = default_cfg(C, True)
    pair = []
    for build, live, ema in ((build_model_2d, w.m2, w.e2), (build_model_3d, w.m3, w.e3)):
        m = build(cfg)[0].cuda()
        shadow = ema.state_dict()["shadow_params"]
        params = [p for p in m.parameters() if p.requires_grad]
        assert len(params) == len(shadow)
        with torch.no_grad():
            for p, s in zip(params, shadow):
                p.copy_(s.view_as(p))
            for (k, dst), (k2, src) in zip(m.named_buffers(), live.named_buffers()):
                assert k == k2
                dst.copy_(src)
        pair.append(m.eval())
    pair[0].net_2d.dropout.p = 0.0
    return pair


def test_no_stale_weight_forms_after_ema_update_and_load():
    w = World()
    t = w.teacher()
    first = [t.predict(w.batch, batched=False, heads="all") for _ in range(2)][-1]    # (the per-image key is recorded now)
    w.step()
    w.e2.update()
    w.e3.update()
    second = t.predict(w.batch, batched=False, heads="all")
    assert t.stats["replays"] >= 2
    for k in ("seg_logit_2d", "seg_logit_3d", "seg_logit_all"):
        assert not torch.equal(first[k], second[k]), k
    with torch.no_grad():
        m2, m3 = fresh_pair(w)
        assert_same(second, eval_per_image(m2, m3, w.batch))
    # ... and after load_state_dict: back to an older shadow
    sd2, sd3 = w.e2.state_dict(), w.e3.state_dict()
    w.step()
    w.e2.update()
    w.e3.update()
    third = t.predict(w.batch, batched=False, heads="all")
    assert not torch.equal(third["seg_logit_2d"], second["seg_logit_2d"])
    v = w.e2.version
    w.e2.load_state_dict(sd2)
    w.e3.load_state_dict(sd3)
    assert w.e2.version == v + 1
    with torch.no_grad():
        m2, m3 = fresh_pair(w)     # (the live buffers moved with the last step: the fresh pair takes the current ones)
        assert_same(t.predict(w.batch, batched=False, heads="all"), eval_per_image(m2, m3, w.batch))


# ------------------------------------------------------------------------------------------------ 6. live buffers
def test_live_batchnorm_buffers_with_a_recorded_key():
    w = World()
    t = w.teacher()
    for _ in range(2):
        t.predict(w.batch, batched=False, heads="all")
    replays = t.stats["replays"]
    rm = w.m2.net_2d.bn1.running_mean.clone()
    w.step()    # train mode: the running statistics move, the shadow does not
    assert not torch.equal(rm, w.m2.net_2d.bn1.running_mean)
    out = t.predict(w.batch, batched=False, heads="all")
    assert t.stats["replays"] == replays + 2 and t.stats["dropped"] == 0
    assert_same(out, by_hand(w, w.batch))


# ------------------------------------------------------------------------------------------------ 7. batched, against G1
def test_batched_and_per_image_match_the_g1_eval_fixtures(golden_dir):
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d, build_model_3d
    from mopa_amd.teacher import Teacher
    cfg = default_cfg(C, True)
    m2 = build_model_2d(cfg)[0]
    m2.load_state_dict({k: det_tensor(k, v.shape) for k, v in m2.state_dict().items()})
    m2.net_2d.dropout.p = 0.0
    m2, m3 = m2.cuda().train(), build_model_3d(cfg)[0].cuda().train()
    x3 = make_batch(9, n=200)[0]["x"]
    t = Teacher(m2, m3)    # the live weights: the predictor of validate() / test.py
    for name in ("pad_eval", "nopad_eval"):
        g = dict(np.load(os.path.join(golden_dir, f"g1_net2dseg_{name}.npz")))
        B = g["img"].shape[0]
        batch = {"img": torch.from_numpy(g["img"]), "img_indices": [g[f"idx{i}"] for i in range(B)], "x": x3}
        dev_batch = dict(batch, img_indices=[cu(g[f"idx{i}"].astype(np.int64)) for i in range(B)])
        runs = {"batched": t.predict(batch, heads="all"), "per image": t.predict(batch, heads="all", batched=False),
                "device indices": t.predict(dev_batch, heads="all")}
        for how, out in runs.items():
            for k, gk in (("seg_logit_2d", "out_seg_logit"), ("seg_logit2_2d", "out_seg_logit2"), ("seg_logit_all", "out_seg_logit_all")):
                ref = g[gk]
                np.testing.assert_allclose(out[k].cpu().numpy(), ref, rtol=1e-3, atol=2e-4 * max(1.0, float(np.abs(ref).max())),
                                           err_msg=f"{name} {how} {k}")
        again = t.predict(batch, heads="all")
        assert_same(again, runs["batched"])
        assert_same(runs["device indices"], runs["batched"])
    assert m2.training and m3.training and m2._calls == 0


# ------------------------------------------------------------------------------------------------ 8. pseudo labels
def scan_batch(seed=21, n=300):
    """prepare_batch_3d(ema_input=True) of two scans whose ROTATED coordinates partly leave the field and whose keep_in mask drops
    points, with the un-augmented image and its indices beside it."""
    from mopa_amd import scanprep as sp
    rng = np.random.Generator(np.random.PCG64(seed))
    a = np.deg2rad(45.0)
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    samples, idx = [], []
    for b in range(2):
        nb = n + 11 * b
        pts = (rng.random((nb, 3)) * np.array([200.0, 200.0, 4.0])).astype(np.float32)   # 200 m x 20 voxels / m < 4096 as loaded
        samples.append({"points": cu(pts), "rot": rot, "transl_u": None, "keep_in": cu(rng.random(nb) < 0.7)})
        idx.append(cu(np.stack([rng.integers(0, H, nb), rng.integers(0, W, nb)], 1).astype(np.int64)))
    batch = sp.prepare_batch_3d(samples, scale=20, full_scale=4096, ema_input=True)
    total = sum(s["points"].shape[0] for s in samples)
    assert batch["ori_x"][0].shape[0] == total and 0 < batch["gather"].numel() < int(sum(int(s["keep_in"].sum()) for s in samples))
    batch["ori_img"] = [torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).cuda() for _ in range(2)]
    batch["ori_img_indices"] = idx
    return batch


@pytest.mark.parametrize("xm", [True, False])
def test_pseudo_labels_equal_the_separate_calls(xm):
    from mopa_amd import pseudo, scanprep as sp
    w = World()
    batch = scan_batch()
    t = w.teacher()
    ps2, ps3 = t.pseudo_labels(batch, xm)
    logits = by_hand(w, {"img": batch["ori_img"], "img_indices": batch["ori_img_indices"], "x": batch["ori_x"]})
    r2, r3 = pseudo.pseudo_labels(logits["seg_logit_2d"], logits["seg_logit_3d"], xm)
    # (batched = one pass over both images; the by-hand recipe is one pass per image: compare the per-image teacher bit for bit)
    q2, q3 = t.pseudo_labels(batch, xm, batched=False)
    for got, ref in ((q2, r2), (q3, r3)):
        assert got.dtype == torch.int64 and got.is_cuda and torch.equal(got, sp.take(batch, ref))
    assert ps2.shape == q2.shape and ps3.shape == q3.shape and ps2.shape[0] == batch["x"][0].shape[0]
    # the default (batched) call: bit for bit the separate calls on the batched pass's own logits, and those logits are the
    # per-image ones in input order within the parity bound of the G1 fixtures (another tile count, maybe another algorithm)
    lb = t.predict(batch, prefer_ori=True)
    b2, b3 = pseudo.pseudo_labels(lb["seg_logit_2d"], lb["seg_logit_3d"], xm)
    assert torch.equal(ps2, sp.take(batch, b2)) and torch.equal(ps3, sp.take(batch, b3))
    np.testing.assert_allclose(lb["seg_logit_2d"].cpu().numpy(), logits["seg_logit_2d"].cpu().numpy(), rtol=1e-3, atol=2e-4)
    assert torch.equal(lb["seg_logit_3d"], logits["seg_logit_3d"])
    # the same compaction from the reference's own keys
    nog = {k: v for k, v in batch.items() if k != "gather"}
    g2, g3 = t.pseudo_labels(nog, xm, batched=False)
    assert torch.equal(g2, q2) and torch.equal(g3, q3)


# ------------------------------------------------------------------------------------------------ 9. no host round trip
def test_pseudo_labels_make_no_host_round_trip():
    """Uses torch.cuda.set_sync_debug_mode("error") (implemented by this build: tests/test_gpu_scanprep.py relies on it too)."""
    w = World()
    batch = scan_batch()
    batch["geometry_3d"] = w.m3.net_3d.geometry(batch["ori_x"][0])
    t = w.teacher()
    for _ in range(3):   # warm-up: eager pass, recording, first replay; workspaces and allocator growth
        ref = t.pseudo_labels(batch, True)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        got = t.pseudo_labels(batch, True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert t.stats["replays"] >= 2
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
