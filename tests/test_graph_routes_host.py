"""Host logic of the launch graphs (frozenbilm_amd/train_graph.py), no GPU: which call takes which route, the get-or-capture
helper with stub graphs, the garbage-collector guard, and what the model keeps per route."""
import gc
import itertools
import types
import warnings

import pytest
import torch

from frozenbilm_amd import train_graph as TG
from frozenbilm_amd.model import DebertaV2Config, DebertaV2ForMaskedLM


def _model():
    cfg = DebertaV2Config(vocab_size=128, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128)
    return DebertaV2ForMaskedLM(cfg, max_feats=4, features_dim=32)


# ------------------------------------------------------------------------------------------------ 1. eligibility
def test_route_for_selects_what_the_three_conditions_of_forward_selected():
    """The specification: the three conditions `DebertaV2ForMaskedLM.forward` tested before the routes moved into one module,
    written out over the same record (`input_ids` is given exactly when `inputs_embeds` is not: forward refuses the rest)."""
    names = {None: None, "inference": TG.INFERENCE, "mlm": TG.MLM, "finetune": TG.FINETUNE}
    flags = [(False, True)] * 7  # inference_graphs, training_graphs, finetune_graphs, training, grad, packed_rows, decoder_rows
    n = 0
    for (inf, trn, ft, training, grad, packed, dec) in itertools.product(*flags):
        model = types.SimpleNamespace(inference_graphs=inf, training_graphs=trn, finetune_graphs=ft, training=training,
                                      packed_rows=packed, decoder_rows=dec, n_ans=0)
        for labels, rows, embeds, (video, video_grad), mlm, n_ans, hidden, attn in itertools.product(
                (False, True), (None, 0, 3), (False, True), ((False, False), (True, False), (True, True)), (False, True),
                (0, 5), (False, True), (False, True)):
            model.n_ans = n_ans
            eager_only = embeds or (grad and video and video_grad)
            spec_inference = (not eager_only and inf and not packed and not dec and rows is not None and not labels
                              and not hidden and not attn and not training and not grad)
            spec_mlm = (not eager_only and trn and not packed and not dec and training and labels and not hidden and not attn
                        and rows is None and not (n_ans and not mlm) and grad)
            spec_finetune = (not eager_only and ft and not packed and not dec and training and rows is not None and not labels
                             and not hidden and not attn and grad and rows > 0)
            held = [k for k, v in (("inference", spec_inference), ("mlm", spec_mlm), ("finetune", spec_finetune)) if v]
            assert len(held) <= 1
            call = TG.Call(ids=not embeds, embeds=embeds, labels=labels, rows=rows, video_grad=video and video_grad, mlm=mlm,
                           hidden_states=hidden, attentions=attn, grad=grad)
            assert TG.route_for(model, call) is names[held[0] if held else None], (vars(model), call)
            n += 1
    assert n == 2 ** 7 * 2 * 3 * 2 * 3 * 2 * 2 * 2 * 2
    assert TG.ROUTES == (TG.INFERENCE, TG.MLM, TG.FINETUNE)


def test_route_for_refuses_a_call_without_token_ids():
    model = types.SimpleNamespace(inference_graphs=True, training_graphs=True, finetune_graphs=True, training=True,
                                  packed_rows=False, decoder_rows=False, n_ans=0)
    call = TG.Call(ids=True, embeds=False, labels=True, rows=None, video_grad=False, mlm=False, hidden_states=False,
                   attentions=False, grad=True)
    assert TG.route_for(model, call) is TG.MLM and TG.route_for(model, call._replace(ids=False)) is None


# ------------------------------------------------------------------------------------------------ 2. get or capture
class StubGraph:
    def __init__(self, fail=False):
        self.pending_backward, self.captured, self.fail = False, 0, fail

    def capture(self):
        if self.fail:
            raise ValueError("no capture today")
        self.captured += 1
        return self


class Harness:
    """a model on the CPU, a stand-in engine, and counters of the warm-ups and builds the helper asked for"""

    def __init__(self, monkeypatch):
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
        self.m, self.eng = _model(), types.SimpleNamespace(dev="cpu")
        self.warm_ups, self.fail = 0, False

    def warm_up(self):
        self.warm_ups += 1

    def get(self, route, conf, eng=None):
        eng = eng or self.eng
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            step = TG._graphed_step(self.m, eng, route, (id(eng),) + tuple(conf), self.warm_up, lambda: StubGraph(self.fail))
        return step, [str(w.message) for w in seen]

    def cache(self, route):
        return self.m.__dict__.get(route.cache, {})


def test_route_records():
    assert [(r.switch, r.cache, r.capacity, r.budgeted) for r in TG.ROUTES] == [
        ("inference_graphs", "_graph_cache", 6, False), ("training_graphs", "_train_graphs", 4, True),
        ("finetune_graphs", "_finetune_graph_cache", 4, True)]
    assert TG.MAX_GRAPHS == 4 and TG.MAX_CAPTURES == 12


@pytest.mark.parametrize("route", TG.ROUTES, ids=lambda r: r.switch)
def test_cache_is_an_lru_of_the_routes_capacity(monkeypatch, route):
    h = Harness(monkeypatch)
    cap = route.capacity
    steps = [h.get(route, (i,))[0] for i in range(cap)]
    assert all(s is not None and s.captured == 1 for s in steps) and h.warm_ups == cap
    assert [k[1] for k in h.cache(route)] == list(range(cap))
    assert h.get(route, (0,))[0] is steps[0] and h.warm_ups == cap  # a hit: no warm-up, no capture, moved to the end
    assert [k[1] for k in h.cache(route)] == list(range(1, cap)) + [0]
    h.get(route, (cap,))  # one more configuration: the least recently used one (1) leaves
    assert [k[1] for k in h.cache(route)] == list(range(2, cap)) + [0, cap] and len(h.cache(route)) == cap
    # a hit does not count as a configuration, and re-capturing a configuration seen before does not either
    h.get(route, (1,))
    assert TG.stats(h.m, route).captures == (cap + 1 if route.budgeted else 0)


@pytest.mark.parametrize("route", TG.ROUTES, ids=lambda r: r.switch)
def test_entries_of_another_engine_are_dropped(monkeypatch, route):
    h = Harness(monkeypatch)
    h.get(route, (1,))
    h.get(route, (2,))
    other = types.SimpleNamespace(dev="cpu")
    step, _ = h.get(route, (1,), eng=other)
    assert list(h.cache(route)) == [(id(other), 1)] and step.captured == 1
    if route.budgeted:  # the count starts over on the new engine
        assert TG.stats(h.m, route).captures == 1 and TG.stats(h.m, route).seen_engine == id(other)


@pytest.mark.parametrize("route", [TG.MLM, TG.FINETUNE], ids=lambda r: r.switch)
def test_the_13th_distinct_configuration_switches_a_budgeted_route_off(monkeypatch, route):
    h = Harness(monkeypatch)
    setattr(h.m, route.switch, True)
    for i in range(12):
        step, said = h.get(route, (i,))
        assert step is not None and not said
    step, said = h.get(route, (3,))  # seen before, evicted since: captured again, not counted
    assert step is not None and not said and TG.stats(h.m, route).captures == 12 and h.warm_ups == 13
    step, said = h.get(route, (12,))
    assert step is None and len(said) == 1 and f"model.{route.switch}: 13 distinct {route.what} configurations" in said[0]
    st = TG.stats(h.m, route)
    assert getattr(h.m, route.switch) is False and st.auto_off is True and st.captures == 13
    assert h.cache(route) == {} and h.warm_ups == 13
    others = [r for r in TG.ROUTES if r is not route]
    assert all(not TG.stats(h.m, r).auto_off and TG.stats(h.m, r).captures == 0 for r in others)


def test_the_inference_route_never_runs_out(monkeypatch):
    h = Harness(monkeypatch)
    h.m.inference_graphs = True
    for i in range(40):
        step, said = h.get(TG.INFERENCE, (i,))
        assert step is not None and not said
    st = TG.stats(h.m, TG.INFERENCE)
    assert h.m.inference_graphs is True and not st.auto_off and st.captures == 0 and len(h.cache(TG.INFERENCE)) == 6


@pytest.mark.parametrize("route", TG.ROUTES, ids=lambda r: r.switch)
def test_a_failed_capture_switches_the_route_off(monkeypatch, route):
    h = Harness(monkeypatch)
    setattr(h.m, route.switch, True)
    h.get(route, (0,))
    h.fail = True
    step, said = h.get(route, (1,))
    assert step is None and len(said) == 1 and "capture failed (ValueError: no capture today)" in said[0]
    assert said[0].startswith(route.failed) and "eager path" in said[0]
    assert getattr(h.m, route.switch) is False and not TG.stats(h.m, route).auto_off
    assert [k[1] for k in h.cache(route)] == [0]  # the failed one is not kept


@pytest.mark.parametrize("route", [TG.MLM, TG.FINETUNE], ids=lambda r: r.switch)
def test_a_forward_before_the_backward_of_the_previous_one_is_refused(monkeypatch, route):
    h = Harness(monkeypatch)
    step, _ = h.get(route, (0,))
    step.pending_backward = True
    with pytest.raises(RuntimeError, match=f"before backward.*model.{route.switch} = False"):
        h.get(route, (0,))
    assert list(h.cache(route).values()) == [step]
    TG.drop_pending_backward(h.m)
    assert h.get(route, (0,))[0] is step


# ------------------------------------------------------------------------------------------------ 3. the collector's guard
@pytest.mark.parametrize("was_on", [True, False])
@pytest.mark.parametrize("raises", [False, True])
def test_gc_guard_restores_the_collectors_state(was_on, raises):
    before = gc.isenabled()
    try:
        (gc.enable if was_on else gc.disable)()
        try:
            with TG.no_gc_during_capture():
                assert not gc.isenabled()
                if raises:
                    raise KeyError("inside")
        except KeyError:
            assert raises
        assert gc.isenabled() is was_on
    finally:
        (gc.enable if before else gc.disable)()


# ------------------------------------------------------------------------------------------------ 4., 5. the model's state
def test_invalidate_drops_the_caches_of_all_routes_and_leaves_the_switches():
    m = _model()
    assert sorted(m._graph_routes) == sorted(r.switch for r in TG.ROUTES)
    m.inference_graphs = m.training_graphs = m.finetune_graphs = True
    for name in ("_graph_cache", "_train_graphs", "_finetune_graph_cache"):
        m.__dict__[name] = {"stale": object()}
    TG.stats(m, TG.FINETUNE).replays = 7
    m.invalidate()
    assert not any(name in m.__dict__ for name in ("_graph_cache", "_train_graphs", "_finetune_graph_cache"))
    assert m.inference_graphs is True and m.training_graphs is True and m.finetune_graphs is True
    assert TG.stats(m, TG.FINETUNE).replays == 7  # (the counters stay: a rebuilt engine starts the capture count over itself)


def test_stats_and_reset_round_trip(monkeypatch):
    h = Harness(monkeypatch)
    for route in TG.ROUTES:
        st = TG.stats(h.m, route)
        assert (st.seen_engine, st.seen, st.auto_off, st.replays, st.captures) == (None, set(), False, 0, 0)
    h.get(TG.MLM, (0,))
    h.get(TG.MLM, (1,))
    TG.stats(h.m, TG.MLM).replays += 2
    st = TG.stats(h.m, TG.MLM)
    assert st.captures == 2 and st.seen == {(0,), (1,)} and st.seen_engine == id(h.eng) and st.replays == 2
    assert TG.stats(h.m, TG.FINETUNE).captures == 0
    h.m.__dict__.pop("_train_graphs")  # popping the pinned name releases the graphs; the counters stay
    assert TG.stats(h.m, TG.MLM).captures == 2
    step, _ = h.get(TG.MLM, (0,))
    assert step.captured == 1 and len(h.cache(TG.MLM)) == 1 and TG.stats(h.m, TG.MLM).captures == 2
    TG.reset(h.m, TG.MLM)
    st = TG.stats(h.m, TG.MLM)
    assert "_train_graphs" not in h.m.__dict__ and (st.captures, st.replays, st.auto_off, st.seen_engine) == (0, 0, False, None)


def test_max_captures_is_read_at_call_time(monkeypatch):
    h = Harness(monkeypatch)
    h.m.finetune_graphs = h.m.inference_graphs = True
    monkeypatch.setattr(TG, "MAX_CAPTURES", 0)  # what the data-parallel workers do to keep a rank on the eager path
    step, said = h.get(TG.FINETUNE, (0,))
    assert step is None and len(said) == 1 and "1 distinct" in said[0] and h.warm_ups == 0
    assert h.m.finetune_graphs is False and TG.stats(h.m, TG.FINETUNE).auto_off is True
    assert h.get(TG.INFERENCE, (0,))[0] is not None and h.m.inference_graphs is True  # no budget there
