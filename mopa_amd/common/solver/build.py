"""``build_optimizer`` with the reference's call shape (``mopa/common/solver/build.py:7-43``, called at
``train_xmuda_mopa.py:131-132``): ``OPTIMIZER.MODEL_xD.TYPE`` picks the flat-buffer class of that name, so the data-parallel
all-reduce, the EMA teacher and the gradient guard come with whichever optimizer the config names.  ``build_scheduler`` is
torch's own and needs nothing from here: every class below is a ``torch.optim.Optimizer``."""
import warnings

import torch

from ...optim import FlatAdam, FlatAdamW, FlatSGD

FLAT_CLASSES = {"Adam": FlatAdam, "AdamW": FlatAdamW, "SGD": FlatSGD}


def build_optimizer(optim_cfg, model, weight_decay=False, model_type="2D", **flat_kwargs):
    """``optim_cfg``: the ``OPTIMIZER.MODEL_2D`` / ``MODEL_3D`` node (``TYPE``, ``BASE_LR``, ``WEIGHT_DECAY`` and an optional
    sub-node named like ``TYPE`` with that optimizer's own arguments: ``Adam.betas``, ``SGD.momentum`` / ``dampening``).
    ``weight_decay`` is accepted and unused, as in the reference (the decay is ``optim_cfg.WEIGHT_DECAY``).

    ``Adam`` / ``AdamW`` / ``SGD`` -> ``FlatAdam`` / ``FlatAdamW`` / ``FlatSGD``; ``flat_kwargs`` (``checkpoint_shapes``,
    ``max_grad_norm``, ``skip_nonfinite``) go to the class, and for ``model_type="3D"`` ``checkpoint_shapes`` defaults to
    ``scn_unet.checkpoint_shapes(model)`` (optimizer state saved in SparseConvNet's weight shapes).  ``''`` warns and returns
    ``None``.  Any other optimizer ``torch.optim`` has is returned as torch's own, with a warning: it trains, but without the
    flat buffers there is no ``all_reduce()``, no ``FlatEMA`` / ``Teacher`` and no guard.  Anything else is a ``ValueError``."""
    name = optim_cfg.TYPE
    if name == "":
        warnings.warn("build_optimizer: TYPE is empty, no optimizer built")
        return None
    extra = dict(optim_cfg.get(name, {}))
    if name in FLAT_CLASSES:
        if model_type == "3D" and "checkpoint_shapes" not in flat_kwargs:
            from ...models.scn_unet import checkpoint_shapes
            flat_kwargs["checkpoint_shapes"] = checkpoint_shapes(model)
        return FLAT_CLASSES[name](model.parameters(), lr=optim_cfg.BASE_LR, weight_decay=optim_cfg.WEIGHT_DECAY, **extra, **flat_kwargs)
    if isinstance(name, str) and isinstance(getattr(torch.optim, name, None), type) \
            and issubclass(getattr(torch.optim, name), torch.optim.Optimizer) and name != "Optimizer":
        if flat_kwargs:
            raise ValueError("build_optimizer: %s are arguments of the flat-buffer optimizers (%s); torch.optim.%s takes none of them"
                             % (", ".join(sorted(flat_kwargs)), ", ".join(FLAT_CLASSES), name))
        warnings.warn("torch.optim.%s is built as it is: the flat-buffer features (data-parallel all_reduce(), FlatEMA / Teacher, "
                      "max_grad_norm / skip_nonfinite) are available with TYPE %s only" % (name, " / ".join(FLAT_CLASSES)))
        return getattr(torch.optim, name)(model.parameters(), lr=optim_cfg.BASE_LR, weight_decay=optim_cfg.WEIGHT_DECAY, **extra)
    raise ValueError("build_optimizer: torch.optim has no optimizer named %r" % (name,))
