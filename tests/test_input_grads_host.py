"""CPU: the host side of `inputs_embeds` -- the argument checks of DebertaV2ForMaskedLM.forward run before the engine is
touched, a well-formed call reaches the engine (which refuses a CPU model), and the BERT model keeps refusing the argument."""
import pytest
import torch

from frozenbilm_amd.model import BertConfig, BertForMaskedLM
from frozenbilm_amd.model.config import DebertaV2Config
from frozenbilm_amd.model.deberta import DebertaV2ForMaskedLM

H = 128


def _tiny():
    c = DebertaV2Config(vocab_size=512, hidden_size=H, num_hidden_layers=3, num_attention_heads=2, intermediate_size=256)
    return DebertaV2ForMaskedLM(c, features_dim=32)


@pytest.mark.parametrize("embeds", [
    torch.zeros(2, H),                          # rank 2
    torch.zeros(1, 2, 5, H),                    # rank 4
    torch.zeros(2, 5, H - 1),                   # last dim != hidden_size
    torch.zeros(2, 5, 2 * H),
], ids=["rank2", "rank4", "narrow", "wide"])
def test_wrong_shape_is_a_value_error(embeds):
    with pytest.raises(ValueError, match="inputs_embeds"):
        _tiny()(inputs_embeds=embeds)


@pytest.mark.parametrize("dtype", [torch.long, torch.int32, torch.bool])
def test_non_floating_dtype_is_a_value_error(dtype):
    with pytest.raises(ValueError, match="floating"):
        _tiny()(inputs_embeds=torch.zeros(2, 5, H, dtype=dtype))


def test_both_or_neither_stay_value_errors():
    m = _tiny()
    with pytest.raises(ValueError):
        m(input_ids=torch.ones(2, 5, dtype=torch.long), inputs_embeds=torch.zeros(2, 5, H))
    with pytest.raises(ValueError):
        m()
    with pytest.raises(ValueError):
        m(video=torch.zeros(2, 3, 32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_well_formed_call_reaches_the_engine(dtype):
    """no NotImplementedError any more: the call gets as far as the engine, which has no CPU fallback"""
    m = _tiny()
    e = torch.zeros(2, 5, H, dtype=dtype, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(inputs_embeds=e, video=torch.zeros(2, 3, 32), labels=torch.full((2, 5), -100))
    m.inference_graphs = m.training_graphs = m.finetune_graphs = True  # the graph switches change nothing about that
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(inputs_embeds=e.detach())


def test_the_argument_checks_come_before_the_engine():
    """a malformed inputs_embeds on a CPU model is a ValueError, not the engine's RuntimeError"""
    m = _tiny()
    with pytest.raises(ValueError):
        m(inputs_embeds=torch.zeros(2, 5, H, dtype=torch.long))
    assert m._engine is None


def test_bert_keeps_refusing_inputs_embeds():
    m = BertForMaskedLM(BertConfig(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=1,
                                   intermediate_size=128, max_position_embeddings=64), features_dim=32, max_feats=4)
    with pytest.raises(NotImplementedError):
        m(inputs_embeds=torch.zeros(2, 5, 64))
    with pytest.raises(ValueError):
        m(input_ids=torch.ones(2, 5, dtype=torch.long), inputs_embeds=torch.zeros(2, 5, 64))
    with pytest.raises(ValueError):
        m()
