"""CPU: the host side of partial fine-tuning (frozenbilm_amd/live_set.py) -- the stage plan as a pure function of (config, live
names, inputs with a gradient), the range builder behind fbl_sumsq_live / fbl_adam_flat_live, the flat layout of an untouched
model, and the refusal of a leaf outside the trainable-by-construction set."""
import pytest
import torch

from frozenbilm_amd.live_set import (flat_layout, live_ranges, refuse_unsupported_leaves, stage_names, stage_of, stage_plan)
from frozenbilm_amd.model import DebertaV2Config, DebertaV2ForMaskedLM
from frozenbilm_amd.model.deberta import flat_order, param_shapes

NL = 4
CFG = DebertaV2Config(vocab_size=512, hidden_size=128, num_hidden_layers=NL, num_attention_heads=2, intermediate_size=256)
ALL = ["emb", "layer0", "conv", "layer1", "layer2", "decoder", "head"]


@pytest.fixture(scope="module")
def model():
    return DebertaV2ForMaskedLM(CFG, features_dim=32)


def test_stage_names_and_stage_of():
    assert stage_names(NL, True) == ALL
    assert stage_names(NL, False) == [s for s in ALL if s != "conv"]
    assert stage_of("lm_predictions.lm_head.LayerNorm.weight", NL) == "head"
    assert stage_of(f"deberta.encoder.layer.{NL - 1}.output.LayerNorm.bias", NL) == "decoder"  # the last layer: the decoder passes
    assert stage_of("deberta.encoder.layer.1.attention.output.adapter.up.weight", NL) == "layer1"
    assert stage_of("deberta.encoder.conv.LayerNorm.weight", NL) == "conv"
    assert stage_of("deberta.encoder.LayerNorm.bias", NL) == "layer0"
    assert stage_of("deberta.embeddings.linear_video.weight", NL) == "emb"
    assert stage_of("deberta.embeddings.LayerNorm.weight", NL) == "emb"


def test_stage_plan_cases(model):
    names = model.trainable_names()
    top = [n for n in names if n.startswith(f"deberta.encoder.layer.{NL - 1}.") and "adapter" in n]
    video = [n for n in names if "linear_video" in n]
    assert top and video
    plan = lambda live, gin=(): list(stage_plan(NL, True, live, gin).running)
    assert plan(names) == ALL                                                   # all live: every stage
    assert plan(top) == ["decoder", "head"]                                     # the top layer's adapters only
    rel = plan(["deberta.encoder.LayerNorm.weight", "deberta.encoder.LayerNorm.bias"])
    assert rel == ALL[1:] and "emb" not in rel                                  # every encoder layer and decoder pass, not emb
    assert plan(video) == ALL                                                   # only linear_video: everything
    assert plan([], ("video",)) == ALL                                          # nothing live but video.requires_grad
    assert plan([], ("embeds",)) == ALL
    assert plan([]) == [] and stage_plan(NL, True, []).lowest is None           # nothing at all: nothing
    assert plan(["lm_predictions.lm_head.LayerNorm.weight"]) == ["head"]
    assert plan(["deberta.encoder.conv.LayerNorm.bias"]) == ALL[2:]
    assert plan(["deberta.encoder.layer.2.output.LayerNorm.weight"] + top) == ["layer2", "decoder", "head"]
    p = stage_plan(NL, True, top)
    assert p.runs("decoder") and p.runs("head") and not p.runs("layer2") and not p.runs("emb") and not p.runs("nonsense")


def test_range_builder():
    order = ["a", "b", "c", "d", "e"]
    numel = {"a": 8, "b": 3, "c": 17, "d": 64, "e": 1}
    offs, total = flat_layout(order, numel)
    assert offs == {"a": 0, "b": 8, "c": 16, "d": 40, "e": 104} and total == 112
    assert live_ranges(order, offs, numel, order) == [(0, 112)]                                       # all live: one range
    assert live_ranges(order, offs, numel, ["a", "c", "e"]) == [(0, 8), (16, 40), (104, 112)]         # alternating: one each
    assert live_ranges(order, offs, numel, ["e", "b", "c"]) == [(8, 40), (104, 112)]                  # merged, sorted
    assert live_ranges(order, offs, numel, []) == []
    for r in (live_ranges(order, offs, numel, s) for s in (["b"], ["c", "d"], ["a", "e"])):
        assert all(b % 8 == 0 and e % 8 == 0 and b < e for b, e in r)
        assert all(r[i][1] < r[i + 1][0] for i in range(len(r) - 1))


def test_model_alternating_parameters_one_range_each(model):
    order = flat_order(CFG, model.trainable_names())
    numel = {n: p.numel() for n, p in model.named_parameters()}
    offs, total = flat_layout(order, numel)
    live = order[::2]
    r = live_ranges(order, offs, numel, live)
    assert len(r) == len(live) and sum(e - b for b, e in r) == sum((numel[n] + 7) // 8 * 8 for n in live)
    assert live_ranges(order, offs, numel, order) == [(0, total)]


def test_untouched_model_layout_is_todays(model):
    """The layout is defined by the constructor flags: for a model nobody toggled it is the one the engine always built --
    requires_grad parameters in flat_order, each padded to 8 floats, one bucket per backward stage -- recomputed here from
    flat_order and param_shapes; and it does not move when flags are toggled."""
    from frozenbilm_amd.engine import Engine

    shapes = param_shapes(CFG, 32, 8, 8, 0)
    by_flag = [n for n, p in model.named_parameters() if p.requires_grad]
    assert model.trainable_names() == by_flag
    order = flat_order(CFG, by_flag)
    want, total = {}, 0
    for n in order:
        want[n] = total
        total += (int(torch.Size(shapes[n]).numel()) + 7) // 8 * 8
    numel = {n: p.numel() for n, p in model.named_parameters()}
    offs, tot = flat_layout(flat_order(CFG, model.trainable_names()), numel)
    assert offs == want and tot == total and list(offs) == order
    ends = {}
    for n in order:
        ends[Engine._bucket_key(None, n)] = want[n] + (numel[n] + 7) // 8 * 8
    assert list(ends) == ["head"] + [k for i in reversed(range(NL)) for k in ((["conv"] if i == 0 else []) + [f"layer{i}"])] \
        + ["relln", "emb"]
    assert sorted(ends.values()) == list(ends.values()) and list(ends.values())[-1] == total
    # toggling flags moves nothing
    p = model.get_param("deberta.embeddings.linear_video.weight")
    p.requires_grad_(False)
    try:
        assert model.trainable_names() == by_flag
    finally:
        p.requires_grad_(True)


def test_refusal_names_the_parameter(model):
    named = dict(model.named_parameters())
    cons = set(model.trainable_names())
    refuse_unsupported_leaves(named, cons)  # an untouched model: fine
    for name in ("deberta.encoder.layer.1.attention.self.query_proj.weight", "lm_predictions.lm_head.dense.weight"):
        named[name].requires_grad_(True)
        try:
            with pytest.raises(NotImplementedError, match=name.replace(".", r"\.")):
                refuse_unsupported_leaves(named, cons)
        finally:
            named[name].requires_grad_(False)
    # the constructor refusals stay as they are
    with pytest.raises(NotImplementedError):
        DebertaV2ForMaskedLM(CFG, features_dim=32, freeze_lm=False)
    with pytest.raises(NotImplementedError):
        DebertaV2ForMaskedLM(CFG, features_dim=32, n_ans=3, freeze_last=False)


def test_bert_trainable_by_construction():
    from frozenbilm_amd.model import BertConfig, BertForMaskedLM

    m = BertForMaskedLM(BertConfig(vocab_size=128, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128,
                                   max_position_embeddings=64), features_dim=16)
    names = m.trainable_names()
    assert names == [n for n, p in m.named_parameters() if p.requires_grad] and any("linear_video" in n for n in names)
    m.get_param("bert.embeddings.linear_video.weight").requires_grad_(False)
    assert m.trainable_names() == names
