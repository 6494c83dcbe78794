"""CPU: LoRA on the frozen Q/K/V projections, host side -- the constructor arguments, the new parameters and their place in the
names / state_dict / flat layout / data-parallel buckets, the refusals, the build_model plumbing, and the semantics the GPU
tests compare against: the oracle run on P[<proj>.weight] = W + s.B@A is the explicit x@W^T + s.(x@A^T)@B^T, position
projections included."""
import types

import pytest
import torch
import torch.nn.functional as F

from frozenbilm_amd.live_set import flat_layout
from frozenbilm_amd.model import BertConfig, BertForMaskedLM, DebertaV2Config, DebertaV2ForMaskedLM, build_model
from frozenbilm_amd.model.deberta import flat_order
from tests.lora_refs import lora_names, lora_tensors, merged_params

NL, H = 3, 128
CFG = DebertaV2Config(vocab_size=512, hidden_size=H, num_hidden_layers=NL, num_attention_heads=2, intermediate_size=256)


def make(**kw):
    return DebertaV2ForMaskedLM(CFG, features_dim=32, **kw)


def layout(m):
    order = flat_order(CFG, m.trainable_names())
    numel = {n: p.numel() for n, p in m.named_parameters()}
    return order, numel, flat_layout(order, numel)


def test_names_shapes_and_initial_values():
    base = make()
    for rank, targets in ((4, ("query_proj", "value_proj")), (64, ("key_proj",)), (1, ("value_proj", "query_proj", "key_proj"))):
        m = make(lora_rank=rank, lora_targets=targets)
        named = dict(m.named_parameters())
        new = [n for n in named if n not in dict(base.named_parameters())]
        want = [f"{mod}.lora_{ab}.weight" for mod in lora_names(NL, targets) for ab in "AB"]
        assert sorted(new) == sorted(want)
        for mod in lora_names(NL, targets):
            A, B = named[mod + ".lora_A.weight"], named[mod + ".lora_B.weight"]
            assert A.shape == (rank, H) and B.shape == (H, rank) and A.requires_grad and B.requires_grad
            assert torch.count_nonzero(B) == 0
            assert A.abs().max().item() <= 1.0 / H ** 0.5 and A.abs().max().item() > 0  # U(-1/sqrt(H), 1/sqrt(H))
        # every pre-existing parameter keeps its initial bits whatever the rank
        for n, p in base.named_parameters():
            assert torch.equal(named[n], p), n
        assert m.lora_scale == 1.0 and m.lora_rank == rank
        assert set(want) <= set(m.trainable_names()) and set(want) <= set(m.state_dict())
    assert make(lora_rank=8, lora_alpha=16).lora_scale == 2.0
    # default targets: query and value
    assert make(lora_rank=2).lora_names() == lora_names(NL, ("query_proj", "value_proj"))


def test_rank_zero_is_todays_model():
    base, m0 = make(), make(lora_rank=0, lora_alpha=32, lora_targets=("key_proj",))
    assert m0.trainable_names() == base.trainable_names()
    assert list(m0.state_dict().keys()) == list(base.state_dict().keys())
    assert [n for n, _ in m0.named_parameters()] == [n for n, _ in base.named_parameters()]
    assert layout(m0)[0] == layout(base)[0] and layout(m0)[2] == layout(base)[2]
    assert m0.lora_names() == [] and m0.lora_rank == 0
    assert make(lora_rank=0, lora_targets=()).lora_rank == 0  # (an empty target set is only refused with a rank)


def test_lora_parameters_sit_in_their_layers_bucket():
    from frozenbilm_amd.engine import Engine

    m = make(lora_rank=4, lora_targets=("query_proj", "key_proj", "value_proj"))
    order, numel, (offs, total) = layout(m)
    ends = {}
    for n in order:  # Engine._build_flat: one bucket per backward stage, ending behind its last parameter
        ends[Engine._bucket_key(None, n)] = offs[n] + (numel[n] + 7) // 8 * 8
    begin, lo = {}, 0
    for key, end in sorted(ends.items(), key=lambda kv: kv[1]):
        begin[key], lo = lo, end
    for mod in lora_names(NL, ("query_proj", "key_proj", "value_proj")):
        i = mod.split(".")[3]
        for leaf in (".lora_A.weight", ".lora_B.weight"):
            n = mod + leaf
            assert begin["layer" + i] <= offs[n] and offs[n] + numel[n] <= ends["layer" + i], n
            assert offs[n] % 8 == 0
    # the layout without the LoRA names is a sub-sequence of the LoRA model's order (nothing else moved relative to the rest)
    rest = [n for n in order if ".lora_" not in n]
    assert rest == layout(make())[0]


def test_bad_arguments_raise_value_error():
    for kw in (dict(lora_rank=65), dict(lora_rank=-1), dict(lora_rank=2.5), dict(lora_rank=4, lora_targets=("dense",)),
               dict(lora_rank=4, lora_targets=("query_proj", "attention.output.dense")), dict(lora_rank=4, lora_targets=())):
        with pytest.raises(ValueError):
            make(**kw)
    with pytest.raises(TypeError):
        make(lora_rank=4, lora_dropout=0.1)  # a merged route cannot apply dropout: the argument does not exist


def test_bert_refuses_lora():
    cfg = BertConfig(vocab_size=256, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    BertForMaskedLM(cfg, features_dim=32, lora_rank=0)
    with pytest.raises(NotImplementedError, match="LoRA"):
        BertForMaskedLM(cfg, features_dim=32, lora_rank=4)


def test_build_model_reads_the_lora_arguments():
    args = types.SimpleNamespace(model_name="deberta-v2-xlarge", features_dim=32, max_feats=10, ds_factor_attn=8, ds_factor_ff=8,
                                 dropout=0.1)
    assert build_model(args, config=CFG).lora_rank == 0
    args.lora_rank, args.lora_alpha, args.lora_targets = 4, 8, ("key_proj",)
    m = build_model(args, config=CFG)
    assert (m.lora_rank, m.lora_scale, m.lora_targets) == (4, 2.0, ("key_proj",))
    assert m.lora_names() == lora_names(NL, ("key_proj",))
    bert = types.SimpleNamespace(model_name="bert-base-uncased", features_dim=32, max_feats=10, ds_factor_attn=0, ds_factor_ff=0,
                                 lora_rank=4)
    with pytest.raises(NotImplementedError, match="LoRA"):
        build_model(bert, config=dict(vocab_size=256, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                      intermediate_size=256, max_position_embeddings=64))


def test_oracle_on_merged_weights_is_the_explicit_low_rank_form(monkeypatch):
    """What the GPU tests compare against: oracle.forward on P' (W + s.B@A in place of W) equals the oracle whose linear layers
    add s.(x@A^T)@B^T explicitly -- for the token projections AND the position projections pos_q / pos_k, which go through
    the same modules (share_att_key).  fp32 mode; both passes of the enhanced mask decoder run (2 layers)."""
    from oracle import deberta_oracle as O
    from tests.golden.make_goldens import _tiny_cfg, synth_batch

    cfg = _tiny_cfg(num_hidden_layers=2)
    P = O.synth_params(cfg, seed=3, std=0.05, ln_jitter=0.1)
    batch = synth_batch(cfg, B=2, L=12, seed=4)
    s = 2.0
    lora = lora_tensors(cfg.hidden_size, 2, 4, ("query_proj", "key_proj", "value_proj"), seed=6, sigma=0.05)
    Pm, _ = merged_params(P, lora, s)
    with torch.no_grad():
        merged = O.forward(Pm, cfg, **batch)
        plain = O.forward(P, cfg, **batch)
    calls = []

    def lin(x, P_, name):
        y = F.linear(x, P_[name + ".weight"], P_.get(name + ".bias"))
        if name + ".lora_A.weight" in lora:
            calls.append((name, tuple(x.shape)))
            y = y + s * ((x @ lora[name + ".lora_A.weight"].t()) @ lora[name + ".lora_B.weight"].t())
        return y

    monkeypatch.setattr(O, "_lin", lin)
    with torch.no_grad():
        explicit = O.forward(P, cfg, **batch)
    # per layer execution (layer 0, then the two decoder passes with layer 1's weights; the oracle skips layer 1's own
    # execution, whose output feeds nothing): q, k, v on the tokens and q, k on the position table
    assert len(calls) == 3 * 5 and sum(1 for _, shp in calls if shp[0] == 1 and shp[1] == 2 * cfg.att_span) == 3 * 2
    d = (merged["logits"] - explicit["logits"]).abs().max().item()
    assert d < 1e-4 * merged["logits"].abs().max().item(), d
    assert abs(merged["loss"].item() - explicit["loss"].item()) < 1e-5
    assert (merged["logits"] - plain["logits"]).abs().max().item() > 1e-2, "the low-rank update made no difference"
