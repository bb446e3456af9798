"""Host-side logic of mopa_amd.teacher: grouping by image size, argument errors, the compaction index, the CPU-model error."""
import numpy as np
import pytest
import torch

from mopa_amd import teacher as T


def test_group_by_size_and_restore_order():
    sizes = [(48, 80), (64, 96), (48, 80), (32, 32), (64, 96)]
    groups = T.group_by_size(sizes)
    assert groups == [[0, 2], [1, 4], [3]]
    assert T.group_by_size(sizes, batched=False) == [[0], [1], [2], [3], [4]]
    assert T.group_by_size([(8, 8)] * 3) == [[0, 1, 2]]
    per_group = [[f"img{i}" for i in g] for g in groups]
    assert T.restore_order(groups, per_group) == [f"img{i}" for i in range(5)]
    with pytest.raises(ValueError):
        T.restore_order(groups, [["a"], ["b", "c"], ["d"]])


def test_plan_2d_inputs_and_argument_errors():
    img = torch.zeros(2, 3, 16, 32)
    idx = [np.zeros((4, 2), np.int64), np.zeros((0, 2), np.int64)]
    imgs, whole, indices, pix, sizes, groups, name = T.plan_2d({"img": img, "img_indices": idx})
    assert whole is img and len(imgs) == 2 and sizes == [(16, 32)] * 2 and groups == [[0, 1]] and pix is None and name == "img_indices"
    # a list of sizes; (1,3,H,W) entries are accepted as the reference passes them
    ori = [torch.zeros(3, 16, 32), torch.zeros(1, 3, 8, 8), torch.zeros(3, 16, 32)]
    plan = T.plan_2d({"img": img, "img_indices": idx, "ori_img": ori, "ori_img_indices": idx + idx[:1]}, prefer_ori=True)
    assert plan[1] is None and plan[4] == [(16, 32), (8, 8), (16, 32)] and plan[5] == [[0, 2], [1]] and plan[6] == "ori_img_indices"
    assert T.plan_2d({"ori_img": ori, "ori_img_indices": idx + idx[:1]})[6] == "ori_img_indices"    # falls back to what is there
    ready = T.plan_2d({"img": img, "point_pix_2d": torch.zeros(4, dtype=torch.int32)})
    assert ready[2] is None and ready[3] is not None
    with pytest.raises(KeyError):       # no image at all
        T.plan_2d({"x": None})
    with pytest.raises(KeyError):       # missing indices
        T.plan_2d({"img": img})
    with pytest.raises(KeyError):
        T.plan_2d({"ori_img": ori, "img_indices": idx}, prefer_ori=True)
    with pytest.raises(IndexError):     # lengths that do not match
        T.plan_2d({"img": img, "img_indices": idx[:1]})
    with pytest.raises(RuntimeError):
        T.plan_2d({"img": torch.zeros(2, 1, 16, 32), "img_indices": idx})
    with pytest.raises(ValueError):     # point_pix_2d cannot address several passes
        T.plan_2d({"img": img, "point_pix_2d": torch.zeros(4, dtype=torch.int32)}, batched=False)


def test_gather_index_equals_keep_then_idxs():
    rng = np.random.Generator(np.random.PCG64(2))
    keeps = [rng.random(n) < 0.6 for n in (50, 1, 33)]
    keeps[1][:] = True
    flags = [rng.random(int(k.sum())) < 0.5 for k in keeps]
    per_point = np.arange(sum(len(k) for k in keeps)) * 3 + 1
    ref, left = [], 0
    for k, i in zip(keeps, flags):
        ref.append(per_point[left:left + len(k)][k][i])
        left += len(k)
    g = T.gather_index([torch.from_numpy(k) for k in keeps], [torch.from_numpy(i) for i in flags], "cpu")
    assert g.dtype == torch.int64 and np.array_equal(per_point[g.numpy()], np.concatenate(ref))
    with pytest.raises(ValueError):
        T.gather_index([torch.from_numpy(keeps[0])], [], "cpu")
    with pytest.raises(TypeError):
        T.gather_index([torch.from_numpy(keeps[0])], [torch.arange(2)], "cpu")


def test_cpu_models_raise_the_usual_error():
    from mopa_amd.config import default_cfg
    from mopa_amd.models.build import build_model_2d, build_model_3d
    cfg = default_cfg(5, True)
    t = T.Teacher(build_model_2d(cfg)[0], build_model_3d(cfg)[0])
    batch = {"img": torch.zeros(1, 3, 16, 16), "img_indices": [np.zeros((1, 2), np.int64)],
             "x": [torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 1)]}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.predict(batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.pseudo_labels(batch, True)
    with pytest.raises(ValueError):
        t.predict(batch, heads="none")
