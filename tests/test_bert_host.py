"""CPU: the BERT variant's host side -- state_dict keys, freeze rule, build_model, the reference's asserts, refusals."""
import pytest
import torch

from frozenbilm_amd.model import BertConfig, BertForMaskedLM, build_model
from oracle.bert_oracle import BertOracleConfig, param_shapes, synth_params
from tests.downstream_fixtures import Args

SMALL = dict(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128,
             max_position_embeddings=64)


def _small(**kw):
    return BertForMaskedLM(BertConfig(**SMALL), features_dim=kw.pop("features_dim", 32), max_feats=4, **kw)


def _ocfg(**kw):
    return BertOracleConfig(**SMALL, features_dim=32, max_feats=4, **kw)


def test_state_dict_keys_and_shapes_are_the_references():
    m = _small()
    sd = m.state_dict()
    ref = param_shapes(_ocfg())
    assert set(sd) == set(ref) | {"bert.embeddings.position_ids"}
    for k, s in ref.items():
        assert tuple(sd[k].shape) == s, k
    assert tuple(sd["bert.embeddings.position_ids"].shape) == (1, 64)
    m2 = _small(n_ans=7)
    assert tuple(m2.state_dict()["answer_embeddings.weight"].shape) == (7, 64)
    assert tuple(m2.state_dict()["answer_bias"].shape) == (7,)


def test_reference_state_dict_loads_with_strict_false():
    """the reference's state dict holds the tied decoder copy and the position_ids buffer on top of the parameters"""
    P = synth_params(_ocfg(), seed=3)
    sd = dict(P)
    sd["cls.predictions.decoder.weight"] = P["bert.embeddings.word_embeddings.weight"]
    sd["cls.predictions.decoder.bias"] = P["cls.predictions.bias"]
    sd["bert.embeddings.position_ids"] = torch.arange(64).expand((1, -1))
    m = _small()
    res = m.load_state_dict(sd, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    m.load_state_dict(sd)  # (strict: the decoder copy is dropped, everything else matches)
    for k, v in P.items():
        assert torch.equal(m.get_param(k).data, v), k


@pytest.mark.parametrize("ft_ln", [True, False])
def test_trainable_set_is_the_freeze_rule(ft_ln):
    m = _small(ft_ln=ft_ln, n_ans=5)
    train = {n for n, p in m.named_parameters() if p.requires_grad}
    want = {"bert.embeddings.linear_video.weight", "bert.embeddings.linear_video.bias"}
    if ft_ln:
        want |= {n for n in param_shapes(_ocfg()) if n.startswith("bert.") and "LayerNorm" in n}
    assert train == want
    assert not any(n.startswith("cls.") for n in train)  # freeze_mlm: the head's LayerNorm too


def _args(**kw):
    d = dict(model_name="bert-base-uncased", features_dim=768, use_video=True, max_feats=10, freeze_lm=True, freeze_mlm=True,
             ft_ln=True, ds_factor_attn=0, ds_factor_ff=0, dropout=0.1, n_ans=0, freeze_last=True, scratch=False)
    d.update(kw)
    return Args(**d)


def test_build_model_for_both_names():
    base = build_model(_args(), config=dict(SMALL))  # (the literal configs are checked below without instantiating them)
    assert isinstance(base, BertForMaskedLM) and base.config.hidden_size == 64
    assert (BertConfig.base().hidden_size, BertConfig.base().num_hidden_layers, BertConfig.base().num_attention_heads,
            BertConfig.base().intermediate_size) == (768, 12, 12, 3072)
    lg = BertConfig.large()
    assert (lg.hidden_size, lg.num_hidden_layers, lg.num_attention_heads, lg.intermediate_size) == (1024, 24, 16, 4096)
    for c in (BertConfig.base(), lg):
        assert (c.vocab_size, c.max_position_embeddings, c.type_vocab_size, c.layer_norm_eps) == (30522, 512, 2, 1e-12)
    m = build_model(_args(model_name="bert-large-uncased", use_video=False, n_ans=3), config=dict(SMALL))
    assert m.features_dim == 0 and m.n_ans == 3
    # "deberta" names keep building the DeBERTa model
    from frozenbilm_amd.model import DebertaV2ForMaskedLM

    d = build_model(_args(model_name="microsoft/deberta-v2-xlarge", ds_factor_attn=8, ds_factor_ff=8),
                    config=dict(vocab_size=128, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128))
    assert isinstance(d, DebertaV2ForMaskedLM)
    with pytest.raises(NotImplementedError):
        build_model(_args(model_name="gpt-neo-1.3B"))


@pytest.mark.parametrize("kw", [dict(ds_factor_attn=8), dict(ds_factor_ff=8), dict(scratch=True)])
def test_reference_asserts(kw):
    with pytest.raises(AssertionError):
        build_model(_args(**kw), config=dict(SMALL))


def test_refusals():
    with pytest.raises(NotImplementedError):
        _small(freeze_lm=False)
    with pytest.raises(NotImplementedError):
        _small(freeze_mlm=False)
    with pytest.raises(NotImplementedError):
        _small(n_ans=4, freeze_last=False)
    m = _small()
    ids = torch.ones(2, 5, dtype=torch.long)
    for kw in (dict(output_attentions=True), dict(inputs_embeds=torch.zeros(2, 5, 64), input_ids=None),
               dict(token_type_ids=torch.ones(2, 5, dtype=torch.long)),
               dict(position_ids=torch.arange(1, 6)[None].expand(2, 5))):
        args = dict(input_ids=ids)
        args.update(kw)
        with pytest.raises(NotImplementedError):
            m(**args)
    from frozenbilm_amd.parallel import GradReducer

    with pytest.raises((NotImplementedError, RuntimeError)):  # (on a CPU-only machine the engine itself refuses first)
        GradReducer.attach(m)


def test_cpu_model_raises_like_the_deberta_model():
    m = _small()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(input_ids=torch.ones(2, 5, dtype=torch.long))
    # token_type_ids of zeros and the default positions are accepted (and then the CPU refusal follows)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(input_ids=torch.ones(2, 5, dtype=torch.long), token_type_ids=torch.zeros(2, 5, dtype=torch.long),
          position_ids=torch.arange(5)[None])


def test_loop_attributes_are_accepted():
    m = _small()
    m.packed_rows = m.inference_graphs = m.training_graphs = True
    assert m.step_seed == 0 and m._reducer is None
    with m.weights_frozen():
        assert m._weights_frozen == 1
