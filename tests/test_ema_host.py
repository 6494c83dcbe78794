"""The host side of the moving average (FusedAdam(..., ema_decay=), frozenbilm_amd/ema.py, loops.ema_weights), without a launch:
constructor validation; the weak registration on the model and `model.ema_weights()` without an average; `loops.ema_weights`
with test doubles -- a null context without the option, one warning per process with the option but no average, the model's
context with both; and (GPU, the engine needs one) the `state_dict()` of a FusedAdam without `ema_decay` has no `fbl_ema` key
and such an optimizer does not register.

Seen on the parent commit: test_constructor_validation fails with ImportError (cannot import name 'ema' from 'frozenbilm_amd'),
test_loops_ema_weights with AttributeError (module 'frozenbilm_amd.loops' has no attribute '_EMA_WARNED'),
test_the_loops_enter_it_around_frozen_weights with AssertionError (main.evaluate opens frozen_weights(model) alone);
test_no_ema_key_by_default stops at its `has_ema` line (AttributeError: 'FusedAdam' object has no attribute 'has_ema')."""
import contextlib
import gc
import warnings
from types import SimpleNamespace

import pytest
import torch


def tiny(bert=False):
    if bert:
        from frozenbilm_amd.model.bert import BertConfig, BertForMaskedLM

        return BertForMaskedLM(BertConfig(vocab_size=64, hidden_size=64, num_hidden_layers=1, num_attention_heads=1,
                                          intermediate_size=128, max_position_embeddings=32), features_dim=32, max_feats=2)
    from frozenbilm_amd.model.config import DebertaV2Config
    from frozenbilm_amd.model.deberta import DebertaV2ForMaskedLM

    c = DebertaV2Config(vocab_size=64, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128,
                        max_position_embeddings=32, position_buckets=8)
    return DebertaV2ForMaskedLM(c, max_feats=2, features_dim=32)


@pytest.mark.parametrize("bert", [False, True], ids=["deberta", "bert"])
def test_constructor_validation(bert):
    from frozenbilm_amd import ema as EMA
    from frozenbilm_amd.optim import FusedAdam

    m = tiny(bert)
    for bad in (0.0, 1.0, -0.5, 1.5, True, False, "0.9", float("nan"), 0, 1, [0.9]):
        with pytest.raises(ValueError):
            FusedAdam(m, lr=1e-3, ema_decay=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError):
            FusedAdam(m, lr=1e-3, ema_decay=0.9, ema_warmup=bad)
    assert "_ema_optimizer" not in m.__dict__  # (a refused constructor registers nothing)
    off = FusedAdam(m, lr=1e-3)
    assert off.ema_decay is None and not off.has_ema and off.ema_updates == 0 and "_ema_optimizer" not in m.__dict__
    with pytest.raises(RuntimeError):
        off.ema_weights()
    with pytest.raises(RuntimeError):
        off.ema_state_dict()
    with pytest.raises(RuntimeError):
        m.ema_weights()  # no optimizer with an average is attached
    opt = FusedAdam(m, lr=1e-3, ema_decay=0.999, ema_warmup=True, param_groups=[dict(params=["*LayerNorm*"], weight_decay=0.0)])
    assert opt.ema_decay == 0.999 and opt.ema_warmup is True and opt.ema_updates == 0 and not opt.has_ema and not opt.ema_open
    assert m.__dict__["_ema_optimizer"]() is opt and EMA.attached(m) is None and not EMA.is_open(m)
    with pytest.raises(RuntimeError):
        m.ema_weights()  # attached, but no step has run: no average yet
    with pytest.raises(RuntimeError):
        opt.ema_weights()
    # the registration is weak: the model does not keep the optimizer alive, and the parameters do not name it
    assert "_ema_optimizer" not in m.state_dict() and len(list(m.named_parameters())) == len(m.state_dict()) - len(list(m.named_buffers()))
    del opt
    gc.collect()
    assert m.__dict__["_ema_optimizer"]() is None and EMA.attached(m) is None and not EMA.is_open(m)
    EMA.refuse_if_open(m, "anything")  # nothing open: no error


class _Double:
    """a model double with an average: counts the entries into its context"""

    def __init__(self, has=True):
        self.entered = self.left = 0
        self.has_ema, self.ema_open = has, False
        from frozenbilm_amd import ema as EMA

        EMA.attach(self, self)

    def ema_weights(self):
        @contextlib.contextmanager
        def scope():
            self.entered += 1
            try:
                yield self
            finally:
                self.left += 1

        return scope()


def test_loops_ema_weights(monkeypatch):
    from frozenbilm_amd import loops

    monkeypatch.setattr(loops, "_EMA_WARNED", False)
    plain = torch.nn.Linear(2, 2)  # a test double: no average, no ema_weights
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # without the option: a null context and not a word, with or without an average
        for args in (SimpleNamespace(), SimpleNamespace(eval_ema=False), None):
            for model in (plain, _Double()):
                ctx = loops.ema_weights(model, args)
                assert isinstance(ctx, contextlib.nullcontext)
                with ctx:
                    pass
    on = SimpleNamespace(eval_ema=True)
    with pytest.warns(UserWarning, match="eval_ema") as rec:  # the option without an average: ONE warning per process
        for model in (plain, _Double(has=False), plain):
            assert isinstance(loops.ema_weights(model, on), contextlib.nullcontext)
    assert len(rec) == 1
    d = _Double()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with loops.ema_weights(d, on) as inside:
            assert inside is d and (d.entered, d.left) == (1, 0)
    assert (d.entered, d.left) == (1, 1)
    assert d.__dict__["_ema_optimizer"]() is d


def test_the_loops_enter_it_around_frozen_weights():
    """main.evaluate, videoqa.evaluate and mc.evaluate open loops.ema_weights(model, args) in front of frozen_weights(model)"""
    import inspect

    from frozenbilm_amd import main, mc, videoqa

    for mod in (main, videoqa, mc):
        src = inspect.getsource(mod.evaluate)
        assert "with ema_weights(model, args), frozen_weights(model)" in src, mod.__name__
        assert mod.ema_weights is __import__("frozenbilm_amd.loops", fromlist=["x"]).ema_weights


@pytest.mark.gpu
def test_no_ema_key_by_default():
    from frozenbilm_amd.optim import FusedAdam

    m = tiny().to("cuda")
    opt = FusedAdam(m, lr=1e-3)
    assert not opt.has_ema
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and "_ema_optimizer" not in m.__dict__
    on = FusedAdam(m, lr=1e-3, ema_decay=0.9)
    assert set(on.state_dict()) == {"state", "param_groups"}  # EMA on, but no average yet: no key either
