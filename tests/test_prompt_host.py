"""CPU: prompt tuning, host side -- the constructor argument, the new parameter and its place in the names / state_dict / flat
layout / data-parallel buckets / parameter groups, the refusals, the build_model plumbing, the text initialisation, the
[MASK]-row helpers of the loops and the eager route under every graph switch."""
import types

import pytest
import torch

from frozenbilm_amd.live_set import flat_layout, stage_of, stage_plan
from frozenbilm_amd.model import BertConfig, BertForMaskedLM, DebertaV2Config, DebertaV2ForMaskedLM, build_model
from frozenbilm_amd.model.deberta import PROMPT_NAME, flat_order

NL, H = 3, 128
CFG = DebertaV2Config(vocab_size=512, hidden_size=H, num_hidden_layers=NL, num_attention_heads=2, intermediate_size=256)
NAME = "deberta.embeddings.prompt_embeddings.weight"


def make(**kw):
    return DebertaV2ForMaskedLM(CFG, features_dim=32, **kw)


def layout(m):
    order = flat_order(CFG, m.trainable_names())
    numel = {n: p.numel() for n, p in m.named_parameters()}
    return order, numel, flat_layout(order, numel)


def test_no_prompt_is_todays_model():
    base, m0 = make(), make(n_prompt=0)
    assert PROMPT_NAME == NAME and m0.n_prompt == 0
    assert [n for n, _ in m0.named_parameters()] == [n for n, _ in base.named_parameters()]
    assert list(m0.state_dict().keys()) == list(base.state_dict().keys())
    assert m0.trainable_names() == base.trainable_names()
    assert layout(m0)[0] == layout(base)[0] and layout(m0)[2] == layout(base)[2]
    for (n, p), (_, q) in zip(base.named_parameters(), m0.named_parameters()):
        assert torch.equal(p, q) and p.requires_grad == q.requires_grad, n


@pytest.mark.parametrize("P", [1, 7])
def test_the_prompt_parameter_and_its_place(P):
    from frozenbilm_amd.engine import Engine

    base, m = make(), make(n_prompt=P)
    named, old = dict(m.named_parameters()), dict(base.named_parameters())
    assert [n for n in named if n not in old] == [NAME] and m.n_prompt == P
    p = named[NAME]
    assert tuple(p.shape) == (P, H) and p.dtype == torch.float32 and p.requires_grad
    assert m._trainable(NAME) and NAME in m.trainable_names() and NAME in m.state_dict()
    # N(0, initializer_range) from a generator of its own (seed 2): reproducible, and no other parameter moved a bit
    want = torch.randn((P, H), generator=torch.Generator().manual_seed(2)) * CFG.initializer_range
    assert torch.equal(p.detach(), want)
    for n, q in old.items():
        assert torch.equal(named[n], q), n
    # the flat order: inside the range of the `emb` stage, next to linear_video; nothing else moved relative to the rest
    order, numel, (offs, total) = layout(m)
    ends = {}
    for n in order:  # Engine._build_flat: one bucket per backward stage, ending behind its last parameter
        ends[Engine._bucket_key(None, n)] = offs[n] + (numel[n] + 7) // 8 * 8
    begin, lo = {}, 0
    for key, end in sorted(ends.items(), key=lambda kv: kv[1]):
        begin[key], lo = lo, end
    assert Engine._bucket_key(None, NAME) == "emb" and stage_of(NAME, NL) == "emb"
    assert begin["emb"] <= offs[NAME] and offs[NAME] + numel[NAME] <= ends["emb"] and offs[NAME] % 8 == 0
    assert begin["emb"] <= offs["deberta.embeddings.linear_video.weight"] < ends["emb"]
    assert [n for n in order if n != NAME] == layout(base)[0]
    # a live prompt alone keeps the embedding stage (hence every stage) in the plan
    assert stage_plan(NL, True, [NAME]).runs("emb")
    assert not stage_plan(NL, True, ["deberta.encoder.layer.0.output.LayerNorm.weight"]).runs("emb")


def test_bad_values_raise_value_error():
    for bad in (-1, 129, 1.5, True, "4", None):
        with pytest.raises(ValueError, match="n_prompt"):
            make(n_prompt=bad)
    assert make(n_prompt=128).n_prompt == 128


def test_bert_refuses_a_prompt():
    cfg = BertConfig(vocab_size=256, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    BertForMaskedLM(cfg, features_dim=32, n_prompt=0)
    with pytest.raises(NotImplementedError, match="n_prompt"):
        BertForMaskedLM(cfg, features_dim=32, n_prompt=4)


def test_build_model_reads_n_prompt():
    args = types.SimpleNamespace(model_name="deberta-v2-xlarge", features_dim=32, max_feats=10, ds_factor_attn=8, ds_factor_ff=8,
                                 dropout=0.1)
    assert build_model(args, config=CFG).n_prompt == 0
    args.n_prompt = 6
    m = build_model(args, config=CFG)
    assert m.n_prompt == 6 and tuple(m.get_param(NAME).shape) == (6, H)
    bert = types.SimpleNamespace(model_name="bert-base-uncased", features_dim=32, max_feats=10, ds_factor_attn=0, ds_factor_ff=0,
                                 n_prompt=4)
    with pytest.raises(NotImplementedError, match="n_prompt"):
        build_model(bert, config=dict(vocab_size=256, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                      intermediate_size=256, max_position_embeddings=64))


def test_init_prompt_from_ids_copies_the_rows():
    m = make(n_prompt=4)
    m._engine = object()  # (stands for a built engine: the call has to drop it)
    ids = torch.tensor([5, 300, 5, 17])
    E = m.get_param("deberta.embeddings.word_embeddings.weight").detach().clone()
    assert m.init_prompt_from_ids(ids) is m
    assert torch.equal(m.get_param(NAME).detach(), E[ids]) and m._engine is None
    assert torch.equal(m.get_param("deberta.embeddings.word_embeddings.weight").detach(), E)
    assert m.get_param(NAME).requires_grad
    for bad in (torch.tensor([1, 2, 3]), torch.tensor([1, 2, 3, 512]), torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.tensor([-1, 2, 3, 4])):
        with pytest.raises(ValueError):
            m.init_prompt_from_ids(bad)
    with pytest.raises(RuntimeError, match="n_prompt"):
        make().init_prompt_from_ids(ids)


def test_mask_row_helpers_shift_by_the_prompt():
    from frozenbilm_amd.videoqa import mask_row_logits, mask_rows

    tok = types.SimpleNamespace(mask_token_id=9)
    ids = torch.tensor([[1, 9, 3, 4], [9, 2, 3, 0], [1, 2, 3, 9]])
    B, Lt, T, P, V = 3, 4, 2, 5, 6
    for use_video in (True, False):
        args = types.SimpleNamespace(max_feats=T, use_video=use_video)
        d = T if use_video else 0
        cols = torch.tensor([1, 0, 3])
        assert mask_rows(ids, tok, args, "cpu").tolist() == [b * (d + Lt) + d + int(c) for b, c in enumerate(cols)]  # as before
        rows = mask_rows(ids, tok, args, "cpu", n_prompt=P)
        S = d + P + Lt
        assert rows.tolist() == [b * S + d + P + int(c) for b, c in enumerate(cols)]
        logits = torch.arange(B * S * V, dtype=torch.float32).view(B, S, V)
        got = mask_row_logits(logits, ids, tok, args, n_prompt=P)
        assert torch.equal(got, logits.view(B * S, V)[rows])
        plain = torch.arange(B * (d + Lt) * V, dtype=torch.float32).view(B, d + Lt, V)
        assert torch.equal(mask_row_logits(plain, ids, tok, args), plain.view(-1, V)[mask_rows(ids, tok, args, "cpu")])


def test_answer_logits_passes_the_models_prompt_length():
    from frozenbilm_amd import videoqa

    tok = types.SimpleNamespace(mask_token_id=9)
    ids = torch.tensor([[1, 9, 3], [9, 2, 3]])
    args = types.SimpleNamespace(max_feats=2, use_video=True)
    S, V = 2 + 4 + 3, 5

    class Fake:  # (no `engine`: the full-logits route)
        n_prompt = 4

        def __call__(self, **feed):
            return {"logits": torch.arange(2 * S * V, dtype=torch.float32).view(2, S, V)}

    got = videoqa.answer_logits(Fake(), tok, ids, args, input_ids=ids)
    want = torch.arange(2 * S * V, dtype=torch.float32).view(2 * S, V)[[0 * S + 6 + 1, 1 * S + 6 + 0]]
    assert torch.equal(got, want)


def test_graph_switches_leave_a_prompt_model_on_the_eager_route():
    from frozenbilm_amd import train_graph as TG

    def call(**kw):
        base = dict(ids=True, embeds=False, labels=False, rows=None, video_grad=False, mlm=False, hidden_states=False,
                    attentions=False, grad=True)
        base.update(kw)
        return TG.Call(**base)

    cases = (("training_graphs", True, call(labels=True, mlm=True), TG.MLM),
             ("finetune_graphs", True, call(rows=4), TG.FINETUNE),
             ("inference_graphs", False, call(rows=4, grad=False), TG.INFERENCE))
    for switch, training, c, route in cases:
        for P in (0, 3):
            m = make(n_prompt=P)
            m.train(training)
            setattr(m, switch, True)
            assert TG.route_for(m, c) is (None if P else route), (switch, P)


def test_state_dict_round_trip_and_reference_checkpoints():
    a, b = make(n_prompt=3), make(n_prompt=3)
    with torch.no_grad():
        a.get_param(NAME).add_(1.0)
    assert not torch.equal(a.get_param(NAME), b.get_param(NAME))
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    b.load_state_dict(sd)
    assert torch.equal(a.get_param(NAME), b.get_param(NAME))
    # a reference checkpoint has no such key: it loads the way a LoRA model loads one, the prompt keeps its initial value
    c = make(n_prompt=3)
    init = c.get_param(NAME).detach().clone()
    res = c.load_state_dict(make().state_dict(), strict=False)
    assert list(res.missing_keys) == [NAME] and not res.unexpected_keys
    assert torch.equal(c.get_param(NAME).detach(), init)
    # trainable-only checkpoints carry it
    from frozenbilm_amd.util.checkpoint import checkpoint_dict

    assert NAME in checkpoint_dict(a, None, 0, None, trainable_only=True)["model"]


def test_layerwise_groups_place_the_prompt_with_the_embeddings_decayed():
    from frozenbilm_amd.param_groups import depth_below_top, layerwise_groups

    m = make(n_prompt=3)
    names = m.trainable_names()
    assert depth_below_top(NAME, NL) == NL == depth_below_top("deberta.embeddings.linear_video.weight", NL)
    groups = layerwise_groups(names, NL, 0.5)
    from frozenbilm_amd.optim import layerwise_param_groups

    assert layerwise_param_groups(m, 0.5) == groups
    mine =[g for g in groups if NAME in g["params"]]
    assert len(mine) == 1 and "weight_decay" not in mine[0] and mine[0]["lr_scale"] == 0.5 ** NL
    assert "deberta.embeddings.linear_video.weight" in mine[0]["params"]
    assert "deberta.embeddings.linear_video.bias" not in mine[0]["params"]
