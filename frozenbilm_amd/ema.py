"""The moving average of the trainable weights, seen from the MODEL: which optimizer keeps it, the `ema_weights()` context of
both models (DeBERTa and BERT share this code), and what a model refuses while that context is open.

The average itself lives in `optim.FusedAdam` (``ema_decay=``): one fp32 buffer with the layout of `engine.flat`, moved inside the
Adam launch (include/fbl_ema.h).  A `FusedAdam` with EMA registers itself WEAKLY on its model -- the model does not keep the
optimizer alive, and a model whose optimizer is gone has no average.
"""
from __future__ import annotations

import weakref

_ATTR = "_ema_optimizer"


def attach(model, optimizer) -> None:
    """called by a FusedAdam with EMA on: `model.ema_weights()` delegates to the last one attached"""
    model.__dict__[_ATTR] = weakref.ref(optimizer)


def attached(model):
    """the optimizer attached to `model` that holds an average right now, or None"""
    ref = getattr(model, "__dict__", {}).get(_ATTR)
    opt = ref() if ref is not None else None
    return opt if (opt is not None and opt.has_ema) else None


def is_open(model) -> bool:
    """inside `ema_weights()`: the flat buffer holds the average, the optimizer's buffer the raw parameters"""
    ref = getattr(model, "__dict__", {}).get(_ATTR)
    opt = ref() if ref is not None else None
    return opt is not None and opt.ema_open


def refuse_if_open(model, what: str) -> None:
    if is_open(model):
        raise RuntimeError(f"{what} inside ema_weights(): the parameters hold the moving average until the context is left, and "
                           "what is written now could not be swapped back")


def weights(model):
    """The context manager behind `model.ema_weights()`: inside it the model computes with the averaged weights."""
    opt = attached(model)
    if opt is None:
        raise RuntimeError("ema_weights(): no FusedAdam(..., ema_decay=) with an average is attached to this model (the average "
                           "starts at the optimizer's first step)")
    return opt.ema_weights()
