"""CPU: deep prompt tuning, host side -- the constructor argument, the per-layer parameters and their place in the names /
state_dict / flat layout / data-parallel buckets / stages / parameter groups, the refusals, the build_model plumbing, the
initialisation from hidden states, the eager route under every graph switch, and the oracle wrappers of
tests/prompt_layers_refs.py against the unwrapped oracle."""
import types

import pytest
import torch

from frozenbilm_amd.live_set import flat_layout, stage_of, stage_plan
from frozenbilm_amd.model import BertConfig, BertForMaskedLM, DebertaV2Config, DebertaV2ForMaskedLM, build_model
from frozenbilm_amd.model.deberta import PROMPT_NAME, flat_order, layer_prompt_name

NL, H = 4, 128
CFG = DebertaV2Config(vocab_size=512, hidden_size=H, num_hidden_layers=NL, num_attention_heads=2, intermediate_size=256)


def make(**kw):
    return DebertaV2ForMaskedLM(CFG, features_dim=32, **kw)


def layout(m):
    order = flat_order(CFG, m.trainable_names())
    numel = {n: p.numel() for n, p in m.named_parameters()}
    return order, numel, flat_layout(order, numel)


def stage_ranges(order, numel, offs):
    """[begin, end) of every data-parallel bucket, as Engine._build_flat forms them: one per backward stage, in flat order"""
    from frozenbilm_amd.engine import Engine

    ends = {}
    for n in order:
        ends[Engine._bucket_key(None, n)] = offs[n] + (numel[n] + 7) // 8 * 8
    out, lo = {}, 0
    for key, end in sorted(ends.items(), key=lambda kv: kv[1]):
        out[key], lo = (lo, end), end
    return out


def test_the_name():
    assert layer_prompt_name(7) == "deberta.encoder.layer.7.prompt.weight"


@pytest.mark.parametrize("kw", [dict(n_prompt=0), dict(n_prompt=5), dict(n_prompt=5, lora_rank=4)], ids=["P0", "P5", "P5-lora"])
def test_depth_one_is_todays_model(kw):
    base, m1 = make(**kw), make(**kw, prompt_depth=1)
    assert m1.prompt_depth == base.prompt_depth == 1 and m1.layer_prompt_names() == []
    assert [n for n, _ in m1.named_parameters()] == [n for n, _ in base.named_parameters()]
    assert not any(".prompt.weight" in n for n, _ in m1.named_parameters())
    assert list(m1.state_dict().keys()) == list(base.state_dict().keys())
    assert m1.trainable_names() == base.trainable_names()
    assert layout(m1)[0] == layout(base)[0] and layout(m1)[2] == layout(base)[2]
    for (n, p), (_, q) in zip(base.named_parameters(), m1.named_parameters()):
        assert torch.equal(p, q) and p.requires_grad == q.requires_grad, n


@pytest.mark.parametrize("P,D,lora", [(1, 2, 0), (4, NL, 0), (4, 3, 4)], ids=["P1-D2", "P4-D4", "P4-D3-lora"])
def test_the_layer_prompts_and_their_place(P, D, lora):
    from frozenbilm_amd.engine import Engine

    base, m = make(n_prompt=P, lora_rank=lora), make(n_prompt=P, prompt_depth=D, lora_rank=lora)
    named, old = dict(m.named_parameters()), dict(base.named_parameters())
    new = [layer_prompt_name(i) for i in range(1, D)]
    assert [n for n in named if n not in old] == new == m.layer_prompt_names() and m.prompt_depth == D
    g = torch.Generator().manual_seed(3)  # N(0, initializer_range) from a generator of its own, layer 1 first
    for n in new:
        p = named[n]
        assert tuple(p.shape) == (P, H) and p.dtype == torch.float32 and p.requires_grad
        assert m._trainable(n) and n in m.trainable_names() and n in m.state_dict()
        assert torch.equal(p.detach(), torch.randn((P, H), generator=g) * CFG.initializer_range), n
    for n, q in old.items():  # no other parameter moved a bit, the layer-0 prompt included
        assert torch.equal(named[n], q), n
    assert PROMPT_NAME in named
    # the flat order: each inside its own layer's range -- the bucket of that layer, where its LoRA factors sit
    order, numel, (offs, total) = layout(m)
    rng = stage_ranges(order, numel, offs)
    for i, n in zip(range(1, D), new):
        key = f"layer{i}"
        assert Engine._bucket_key(None, n) == key
        assert stage_of(n, NL) == (key if i < NL - 1 else "decoder")
        b, e = rng[key]
        assert b <= offs[n] and offs[n] + numel[n] <= e and offs[n] % 8 == 0, (n, offs[n], b, e)
        mates = [k for k in order if k.startswith(f"deberta.encoder.layer.{i}.") and k != n]
        assert mates and all(b <= offs[k] < e for k in mates)
        if lora:
            assert any(".lora_" in k for k in mates)
    assert [n for n in order if n not in new] == layout(base)[0]  # nothing else moved relative to the rest
    # a live layer prompt alone: its own stage is the lowest that runs
    for i, n in zip(range(1, D), new):
        plan = stage_plan(NL, True, [n])
        low = f"layer{i}" if i < NL - 1 else "decoder"
        assert plan.running[0] == low and plan.runs("head") and not plan.runs("emb") and not plan.runs(f"layer{i - 1}")


def test_bad_values_raise_value_error():
    for bad in (0, -1, NL + 1, 1.5, True, "2", None):
        with pytest.raises(ValueError, match="prompt_depth"):
            make(n_prompt=4, prompt_depth=bad)
    for D in (2, NL):
        with pytest.raises(ValueError, match="n_prompt"):
            make(prompt_depth=D)
        with pytest.raises(ValueError, match="n_prompt"):
            make(n_prompt=0, prompt_depth=D)
    assert make(prompt_depth=1).prompt_depth == 1  # no slots, depth 1: the reference's model
    assert make(n_prompt=128, prompt_depth=NL).prompt_depth == NL


def test_bert_refuses():
    cfg = BertConfig(vocab_size=256, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=64)
    BertForMaskedLM(cfg, features_dim=32, prompt_depth=1)
    with pytest.raises(NotImplementedError, match="prompt_depth"):
        BertForMaskedLM(cfg, features_dim=32, prompt_depth=2)
    with pytest.raises(NotImplementedError, match="prompt_depth"):
        BertForMaskedLM(cfg, features_dim=32, n_prompt=4, prompt_depth=2)


def test_build_model_reads_prompt_depth():
    args = types.SimpleNamespace(model_name="deberta-v2-xlarge", features_dim=32, max_feats=10, ds_factor_attn=8, ds_factor_ff=8,
                                 dropout=0.1, n_prompt=6)
    assert build_model(args, config=CFG).prompt_depth == 1
    args.prompt_depth = 3
    m = build_model(args, config=CFG)
    assert m.prompt_depth == 3 and tuple(m.get_param(layer_prompt_name(2)).shape) == (6, H)
    args.prompt_depth = NL + 1
    with pytest.raises(ValueError, match="prompt_depth"):
        build_model(args, config=CFG)
    bert = types.SimpleNamespace(model_name="bert-base-uncased", features_dim=32, max_feats=10, ds_factor_attn=0, ds_factor_ff=0,
                                 prompt_depth=2)
    with pytest.raises(NotImplementedError, match="prompt_depth"):
        build_model(bert, config=dict(vocab_size=256, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                      intermediate_size=256, max_position_embeddings=64))


def test_parameter_groups_put_each_at_its_layers_depth():
    from frozenbilm_amd.optim import layerwise_param_groups
    from frozenbilm_amd.param_groups import depth_below_top, resolve

    m = make(n_prompt=3, prompt_depth=NL)
    groups = layerwise_param_groups(m, 0.5)
    names = resolve(groups, m.trainable_names())
    for i in range(1, NL):
        n = layer_prompt_name(i)
        k = [j for j, g in enumerate(names) if n in g]
        assert len(k) == 1
        grp = groups[k[0]]
        d = NL - 1 - i
        assert depth_below_top(n, NL) == d
        assert grp.get("lr_scale", 1.0) == 0.5 ** d and "weight_decay" not in grp  # decayed, like prompt_embeddings
        mate = f"deberta.encoder.layer.{i}.output.adapter.down.weight"
        assert mate in names[k[0]]  # the group of its layer's decayed weights
    kp = [j for j, g in enumerate(names) if PROMPT_NAME in g][0]
    assert "weight_decay" not in groups[kp] and groups[kp]["lr_scale"] == 0.5 ** NL


def test_state_dict_round_trip_and_checkpoints_without_the_keys():
    from frozenbilm_amd.util.checkpoint import checkpoint_dict

    D = 3
    a, b = make(n_prompt=3, prompt_depth=D), make(n_prompt=3, prompt_depth=D)
    new = a.layer_prompt_names()
    with torch.no_grad():
        for k, n in enumerate(new):
            a.get_param(n).add_(1.0 + k)
    assert not any(torch.equal(a.get_param(n), b.get_param(n)) for n in new)
    b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    assert all(torch.equal(a.get_param(n), b.get_param(n)) for n in new)
    # the checkpoint of a shallow model has no such keys: it loads, the rows keep their initial value
    c = make(n_prompt=3, prompt_depth=D)
    init = {n: c.get_param(n).detach().clone() for n in new}
    res = c.load_state_dict(make(n_prompt=3).state_dict(), strict=False)
    assert list(res.missing_keys) == new and not res.unexpected_keys
    assert all(torch.equal(c.get_param(n).detach(), init[n]) for n in new)
    # trainable-only checkpoints carry them
    sd = checkpoint_dict(a, None, 0, None, trainable_only=True)["model"]
    assert all(n in sd and torch.equal(sd[n], a.get_param(n)) for n in new)
    assert "deberta.embeddings.word_embeddings.weight" not in sd


def test_init_prompt_layers_from_hidden():
    P, D, T, B, S = 3, NL, 2, 4, 11
    m = make(n_prompt=P, prompt_depth=D)
    m._engine = object()  # (stands for a built engine: the call has to drop it)
    g = torch.Generator().manual_seed(7)
    hs = tuple(torch.randn(B, S, H, generator=g) for _ in range(NL + 1))
    shallow = m.get_param(PROMPT_NAME).detach().clone()
    assert m.init_prompt_layers_from_hidden(hs, T) is m and m._engine is None
    for i in range(1, D):
        w = m.get_param(layer_prompt_name(i))
        assert torch.equal(w.detach(), hs[i][:, T:T + P].mean(0)) and w.requires_grad
    assert torch.equal(m.get_param(PROMPT_NAME).detach(), shallow)
    m2 = make(n_prompt=P, prompt_depth=2)  # the first D tensors are enough; T = 0: no video slots
    m2.init_prompt_layers_from_hidden(hs[:2], 0)
    assert torch.equal(m2.get_param(layer_prompt_name(1)).detach(), hs[1][:, :P].mean(0))
    with pytest.raises(ValueError):
        m.init_prompt_layers_from_hidden(hs[:D - 1], T)
    with pytest.raises(ValueError):
        m.init_prompt_layers_from_hidden(hs, S - P + 1)
    with pytest.raises(ValueError):
        m.init_prompt_layers_from_hidden(hs, -1)
    with pytest.raises(ValueError):
        m.init_prompt_layers_from_hidden(tuple(h[..., :64] for h in hs), T)
    with pytest.raises(RuntimeError, match="prompt_depth"):
        make(n_prompt=P).init_prompt_layers_from_hidden(hs, T)


def test_graph_switches_leave_a_deep_prompt_model_on_the_eager_route():
    from frozenbilm_amd import train_graph as TG

    def call(**kw):
        base = dict(ids=True, embeds=False, labels=False, rows=None, video_grad=False, mlm=False, hidden_states=False,
                    attentions=False, grad=True)
        base.update(kw)
        return TG.Call(**base)

    cases = (("training_graphs", True, call(labels=True, mlm=True)), ("finetune_graphs", True, call(rows=4)),
             ("inference_graphs", False, call(rows=4, grad=False)))
    for switch, training, c in cases:
        for D in (2, NL):
            m = make(n_prompt=3, prompt_depth=D)
            m.train(training)
            setattr(m, switch, True)
            assert TG.route_for(m, c) is None, (switch, D)


# ------------------------------------------------------------------------------------------------ the oracle wrappers
@pytest.mark.parametrize("T,D", [(3, 2), (3, 3), (0, 3)], ids=["T3-D2", "T3-DnL", "T0-DnL"])
def test_wrapped_oracle_reproduces_the_unwrapped_one_on_its_own_rows(T, D):
    """B = 1: overwriting the prompt slots of hs[i] with hs[i]'s own rows is the identity, so the wrapped oracle must give the
    unwrapped one's logits and hidden states exactly; a wrapper that cut the wrong rows or missed a call would not.  With other
    rows the logits move, and the originals are back in place afterwards."""
    from oracle import deberta_oracle as O
    from tests.prompt_layers_refs import deep_prompts
    from tests.test_gpu_input_grads import _batch, _cfg, _params

    P, Lt = 4, 6
    cfg = _cfg(T)
    nL = cfg.num_hidden_layers
    Pd = _params(cfg, 91)
    b = _batch(cfg, T, P + Lt, seed=31, B=1, labels=False)  # (the slots are ordinary text positions of the plain oracle)
    if not T:
        b.pop("video"), b.pop("video_mask")
    # (_batch pads its last sample, here the only one: with the text valid, rows outside the slots read the slots as keys and
    # every layer's prompt has a gradient)
    b["attention_mask"][:] = 1
    b["input_ids"][b["input_ids"] == 0] = 7
    layer0, emd0 = O.layer, O.emd
    with torch.no_grad():
        ref = O.forward(Pd, cfg, **b, return_hidden=True)
        own = {i: ref["hidden_states"][i][0, T:T + P].clone() for i in range(1, D)}
        with deep_prompts(own, T, nL):
            assert O.layer is not layer0 and O.emd is not emd0
            got = O.forward(Pd, cfg, **b, return_hidden=True)
        assert torch.equal(got["logits"], ref["logits"])
        assert all(torch.equal(h, k) for h, k in zip(got["hidden_states"], ref["hidden_states"]))
        other = {i: v + 0.5 for i, v in own.items()}
        with deep_prompts(other, T, nL):
            moved = O.forward(Pd, cfg, **b)
        assert (moved["logits"] - ref["logits"]).abs().max().item() > 1e-3
    assert O.layer is layer0 and O.emd is emd0
    # the gradient reaches the leaves, and nothing flows from the slots into the layer below: with D == nL, hs[nL-1]'s own
    # slot rows feed nothing at all once they are overwritten
    leaves = {i: v.clone().requires_grad_() for i, v in own.items()}
    with deep_prompts(leaves, T, nL):
        out = O.forward(Pd, cfg, **b)
    out["logits"].square().sum().backward()
    assert all(v.grad is not None and v.grad.norm().item() > 0 for v in leaves.values())
