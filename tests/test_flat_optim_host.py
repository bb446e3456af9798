"""The host side of FlatSGD / FlatAdamW and of build_optimizer (mopa_amd/optim.py, mopa_amd/common/solver/build.py): dispatch by
TYPE, checkpoints in the layout of the installed torch optimizers in both directions, argument errors.  No GPU: the kernels are
in tests/test_gpu_flat_optim.py."""
import warnings

import pytest
import torch

from mopa_amd.common.solver.build import build_optimizer
from mopa_amd.config import Node
from mopa_amd.optim import FlatAdam, FlatAdamW, FlatOptimizer, FlatSGD
from mopa_amd.pseudo import FlatEMA

SHAPES = ((7, 3), (130,), (5, 5, 5), (1,))


def _params(seed=0):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.ps = torch.nn.ParameterList(_params())


def _cfg(type_, **sub):
    node = Node(TYPE=type_, BASE_LR=0.05, WEIGHT_DECAY=0.02)
    if sub:
        node[type_] = Node(**sub)
    return node


# ------------------------------------------------------------------------------------------------ build_optimizer
def test_build_optimizer_gives_the_flat_class_of_that_name():
    with warnings.catch_warnings():
        warnings.simplefilter("error")            # no warning on the supported names
        adam = build_optimizer(_cfg("Adam", betas=(0.8, 0.99)), _Model())
        adamw = build_optimizer(_cfg("AdamW", betas=(0.7, 0.9), eps=1e-6), _Model(), weight_decay=True)
        sgd = build_optimizer(_cfg("SGD", momentum=0.9, dampening=0.1), _Model(), max_grad_norm=3.0, skip_nonfinite=True)
        plain = build_optimizer(_cfg("SGD"), _Model())
    assert type(adam) is FlatAdam and type(adamw) is FlatAdamW and type(sgd) is FlatSGD and type(plain) is FlatSGD
    for opt in (adam, adamw, sgd, plain):
        assert isinstance(opt, FlatOptimizer) and isinstance(opt, torch.optim.Optimizer)
        g = opt.param_groups[0]
        assert g["lr"] == 0.05 and g["weight_decay"] == 0.02 and len(g["params"]) == len(SHAPES)
    assert adam.param_groups[0]["betas"] == (0.8, 0.99)
    assert adamw.param_groups[0]["betas"] == (0.7, 0.9) and adamw.param_groups[0]["eps"] == 1e-6
    assert sgd.param_groups[0]["momentum"] == 0.9 and sgd.param_groups[0]["dampening"] == 0.1
    assert sgd.max_grad_norm == 3.0 and sgd.skip_nonfinite is True and plain.max_grad_norm is None
    assert plain.param_groups[0]["momentum"] == 0 and plain.momentum_buf is None


def test_build_optimizer_checkpoint_shapes_pass_through():
    shapes = [(3, 7), None, (125,), None]
    opt = build_optimizer(_cfg("SGD", momentum=0.5), _Model(), checkpoint_shapes=shapes)
    assert opt._ckpt_shapes == shapes


def test_build_optimizer_other_names():
    with pytest.warns(UserWarning):
        assert build_optimizer(_cfg(""), _Model()) is None
    with pytest.warns(UserWarning, match="flat-buffer"):
        opt = build_optimizer(_cfg("Adagrad"), _Model())
    assert type(opt) is torch.optim.Adagrad and opt.param_groups[0]["lr"] == 0.05 and opt.param_groups[0]["weight_decay"] == 0.02
    with pytest.raises(ValueError):
        build_optimizer(_cfg("Nope"), _Model())


# ------------------------------------------------------------------------------------------------ checkpoints, both directions
def _torch_stepped(cls, **kw):
    ref = cls(_params(), lr=1e-2, **kw)
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        for p in ref.param_groups[0]["params"]:
            p.grad = torch.randn(p.shape, generator=gen)
        ref.step()
    return ref


@pytest.mark.parametrize("flat_cls,torch_cls,kw,keys", (
    (FlatSGD, torch.optim.SGD, dict(momentum=0.9, dampening=0.1, weight_decay=0.01), ("momentum_buffer",)),
    (FlatSGD, torch.optim.SGD, dict(momentum=0.9, nesterov=True), ("momentum_buffer",)),
    (FlatAdamW, torch.optim.AdamW, dict(weight_decay=0.1, betas=(0.8, 0.99)), ("step", "exp_avg", "exp_avg_sq"))))
def test_checkpoints_move_between_torch_and_the_flat_class(flat_cls, torch_cls, kw, keys):
    opt = flat_cls(_params(), lr=1e-2, **kw)
    fresh = torch_cls(_params(), lr=1e-2, **kw)
    sd0 = opt.state_dict()
    assert sd0["state"] == {}, "state before any step"
    assert set(sd0["param_groups"][0]) == set(fresh.state_dict()["param_groups"][0])
    assert sd0["param_groups"][0]["params"] == list(range(len(SHAPES)))
    for k, v in fresh.state_dict()["param_groups"][0].items():
        assert sd0["param_groups"][0][k] == v, k
    ref = _torch_stepped(torch_cls, **kw)
    want = ref.state_dict()
    opt.load_state_dict(want)
    got = opt.state_dict()
    assert set(got["state"]) == set(want["state"]) == set(range(len(SHAPES)))
    for i in want["state"]:
        assert set(got["state"][i]) == set(want["state"][i]) == set(keys)
        for k in keys:
            a, b = got["state"][i][k], want["state"][i][k]
            assert a.shape == b.shape and torch.equal(a.float(), b.float()), (i, k)
    back = torch_cls(_params(), lr=1e-2, **kw)
    back.load_state_dict(got)                    # ... and torch's own optimizer takes ours
    for i, p in enumerate(back.param_groups[0]["params"]):
        for k in keys:
            assert torch.equal(torch.as_tensor(back.state[p][k]).float(), torch.as_tensor(want["state"][i][k]).float())
    if flat_cls is FlatSGD:
        assert opt._first is False, "loaded buffers mean: not the first step"
        opt.load_state_dict(sd0)                 # an empty checkpoint makes the next step the first again
        assert opt._first is True and opt.state_dict()["state"] == {} and not bool(opt.momentum_buf.any())
    else:
        assert opt.t == 3


def test_sgd_without_momentum_has_no_state():
    opt = FlatSGD(_params(), lr=1e-2)
    assert opt.state_dict()["state"] == {} and opt.momentum_buf is None
    ref = _torch_stepped(torch.optim.SGD)
    opt.load_state_dict(ref.state_dict())
    assert opt.state_dict()["state"] == {} and opt.momentum_buf is None
    torch.optim.SGD(_params(), lr=1e-2).load_state_dict(opt.state_dict())


def test_checkpoint_shapes_shape_the_momentum_buffers():
    shapes = [(3, 7), None, (125,), None]
    opt = FlatSGD(_params(), lr=1e-2, momentum=0.9, checkpoint_shapes=shapes)
    opt.load_state_dict(_torch_stepped(torch.optim.SGD, momentum=0.9).state_dict())
    got = [tuple(opt.state_dict()["state"][i]["momentum_buffer"].shape) for i in range(4)]
    assert got == [(3, 7), (130,), (125,), (1,)]


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_errors():
    with pytest.raises(ValueError, match="[Nn]esterov"):
        FlatSGD(_params(), lr=1e-2, nesterov=True)
    with pytest.raises(ValueError, match="[Nn]esterov"):
        FlatSGD(_params(), lr=1e-2, momentum=0.9, dampening=0.1, nesterov=True)
    for cls in (FlatSGD, FlatAdamW):
        with pytest.raises(ValueError, match="max_grad_norm"):
            cls(_params(), max_grad_norm=0.0)
        with pytest.raises(ValueError, match=cls.__name__ + " got no parameters"):
            cls([])
    with pytest.raises(ValueError, match="FlatAdam got no parameters"):
        FlatAdam([])


@pytest.mark.parametrize("make", (lambda: FlatSGD(_params(), lr=1e-2, momentum=0.9),
                                  lambda: FlatSGD(_params(), lr=1e-2, skip_nonfinite=True),
                                  lambda: FlatAdamW(_params(), lr=1e-2),
                                  lambda: FlatAdamW(_params(), lr=1e-2, max_grad_norm=1.0)))
def test_step_on_the_cpu_is_an_error(make):
    opt = make()
    before = opt.flat.clone()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(opt.flat, before)


def test_flat_ema_over_flat_sgd():
    shapes = [(3, 7), None, (125,), None]
    opt = FlatSGD(_params(), lr=1e-2, momentum=0.9, checkpoint_shapes=shapes)
    sd = FlatEMA(opt, 0.99).state_dict()
    assert [tuple(t.shape) for t in sd["shadow_params"]] == [(3, 7), (130,), (125,), (1,)]
    for t, p in zip(sd["shadow_params"], opt.params):
        assert torch.equal(t.reshape(-1), p.detach().reshape(-1))
