"""CPU: frozenbilm_amd/param_groups.py -- names, patterns and tensors resolved into groups and the errors; the segments of live
sets that cut through groups; layerwise_groups on a 3-layer name list (scales, the two special cases, the decay split, the BERT
names); lr_scale; the state-dict index map of three groups.  Pure host logic: no tensor, no GPU.

Seen on the parent commit: every test errors in the `PG` fixture -- ImportError: cannot import name 'param_groups' from
'frozenbilm_amd'."""
import pytest

L0, L1, L2 = ("deberta.encoder.layer.%d." % i for i in range(3))
AD = "attention.output.adapter."
NAMES = [
    "deberta.embeddings.linear_video.weight", "deberta.embeddings.linear_video.bias",
    "deberta.embeddings.LayerNorm.weight", "deberta.embeddings.LayerNorm.bias",
    L0 + AD + "down.weight", L0 + AD + "down.bias", L0 + "output.LayerNorm.weight",
    "deberta.encoder.conv.LayerNorm.weight", "deberta.encoder.conv.LayerNorm.bias",
    L1 + AD + "down.weight", L1 + AD + "down.bias", L1 + "output.LayerNorm.weight",
    L2 + AD + "down.weight", L2 + AD + "down.bias", L2 + "output.LayerNorm.weight",
    "deberta.encoder.LayerNorm.weight", "deberta.encoder.LayerNorm.bias",
    "lm_predictions.lm_head.LayerNorm.weight",
]


@pytest.fixture(scope="module")
def PG():
    from frozenbilm_amd import param_groups

    return param_groups


def test_names_patterns_and_tensors(PG):
    tensors = {n: object() for n in NAMES}  # stand-ins: resolve() only looks at id()
    ids = {id(t): n for n, t in tensors.items()}
    got = PG.resolve([dict(params=[]), dict(params=["*LayerNorm*"]), dict(params=[tensors[NAMES[1]], L2 + AD + "down.bias"])],
                     NAMES, ids)
    assert got[1] == [n for n in NAMES if "LayerNorm" in n]
    assert got[2] == [NAMES[1], L2 + AD + "down.bias"]  # in the order of the trainable set
    assert got[0] == [n for n in NAMES if n not in got[1] and n not in got[2]]  # what nothing names joins group 0
    assert sorted(sum(got, [])) == sorted(NAMES)  # every parameter in exactly one group
    assert PG.resolve([], NAMES) == [NAMES]  # no specification: one group
    assert PG.resolve([dict(params="*.bias")], NAMES)[0] == NAMES  # a single pattern, not in a list
    assert PG.group_of(got)[NAMES[1]] == 2 and PG.group_of(got)[NAMES[0]] == 0
    # the errors
    with pytest.raises(ValueError, match="twice"):
        PG.resolve([dict(params=[NAMES[0]]), dict(params=[NAMES[0]])], NAMES)
    with pytest.raises(ValueError, match="twice"):
        PG.resolve([dict(params=["*LayerNorm*"]), dict(params=["*.bias"])], NAMES)  # the LayerNorm biases
    with pytest.raises(ValueError, match="twice"):
        PG.resolve([dict(params=[NAMES[0], tensors[NAMES[0]]])], NAMES, ids)
    with pytest.raises(ValueError, match="not trainable"):
        PG.resolve([dict(params=["deberta.encoder.layer.0.intermediate.dense.weight"])], NAMES)
    with pytest.raises(ValueError, match="meets no"):
        PG.resolve([dict(params=["*intermediate*"])], NAMES)
    with pytest.raises(ValueError, match="tensor"):
        PG.resolve([dict(params=[object()])], NAMES, ids)
    with pytest.raises(ValueError, match="tensor"):
        PG.resolve([dict(params=[tensors[NAMES[0]]])], NAMES[1:], ids)  # a tensor of the model outside the trainable set


def test_segments_for_live_sets_that_cut_through_groups(PG):
    order = ["a", "b", "c", "d", "e"]
    numel = dict(a=8, b=5, c=16, d=3, e=24)
    offsets, total = {}, 0
    for n in order:
        offsets[n] = total
        total += (numel[n] + 7) // 8 * 8
    assert total == 64
    gof = dict(a=0, b=0, c=1, d=1, e=0)
    seg = lambda live: PG.segments(order, offsets, numel, live, gof)  # noqa: E731
    assert seg(order) == [(0, 16, 0), (16, 40, 1), (40, 64, 0)]  # neighbours of one group merge, padding included
    assert seg(["a", "c", "e"]) == [(0, 8, 0), (16, 32, 1), (40, 64, 0)]
    assert seg(["b", "c"]) == [(8, 16, 0), (16, 32, 1)]  # adjacent, two groups: two segments
    assert seg(["d"]) == [(32, 40, 1)] and seg([]) == []
    assert seg(["e", "a"]) == [(0, 8, 0), (40, 64, 0)]  # sorted by offset whatever the order given
    gof2 = dict(a=0, b=1, c=0, d=1, e=0)
    assert PG.segments(order, offsets, numel, order, gof2) == [(0, 8, 0), (8, 16, 1), (16, 32, 0), (32, 40, 1), (40, 64, 0)]


def test_layerwise_groups(PG):
    gs = PG.layerwise_groups(NAMES, 3, 0.5)
    PG.check_groups(gs)
    assert "lr_scale" not in gs[0] and "weight_decay" not in gs[0]
    members = PG.resolve(gs, NAMES)
    assert sorted(sum(members, [])) == sorted(NAMES)
    scale = {n: g.get("lr_scale", 1.0) for g in gs for n in g["params"]}
    undecayed = {n for g in gs if g.get("weight_decay") == 0.0 for n in g["params"]}
    # the head, the decoder passes (the top layer) and the relative-position LayerNorm: scale 1
    for n in NAMES:
        if n.startswith(L2) or n.startswith("lm_predictions.") or n.startswith("deberta.encoder.LayerNorm."):
            assert scale[n] == 1.0, n
    # every stage below: the scale above it times decay; conv counts with layer 0; the embedding stage one below layer 0
    for n in NAMES:
        if n.startswith(L1):
            assert scale[n] == 0.5, n
        if n.startswith(L0) or n.startswith("deberta.encoder.conv."):
            assert scale[n] == 0.25, n
        if n.startswith("deberta.embeddings."):
            assert scale[n] == 0.125, n
    # each depth splits by the no_decay substrings
    assert undecayed == {n for n in NAMES if "LayerNorm" in n or "bias" in n}
    assert len(gs) == 8  # four depths x (decayed, undecayed)
    assert [g.get("lr_scale", 1.0) for g in gs] == [1.0, 1.0, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125]
    assert gs[0]["params"] == [L2 + AD + "down.weight"]
    # other substrings; decay 1 keeps every rate; a bad decay is refused
    only_ln = PG.layerwise_groups(NAMES, 3, 1.0, no_decay=("LayerNorm",))
    assert {n for g in only_ln if g.get("weight_decay") == 0.0 for n in g["params"]} == {n for n in NAMES if "LayerNorm" in n}
    assert all(g.get("lr_scale", 1.0) == 1.0 for g in only_ln)
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            PG.layerwise_groups(NAMES, 3, bad)
    # only LayerNorms train: group 0, the decayed group of the top, stays (empty) so that it is the rate the others scale
    ln = [n for n in NAMES if "LayerNorm" in n]
    g_ln = PG.layerwise_groups(ln, 3, 0.5)
    assert g_ln[0]["params"] == [] and "lr_scale" not in g_ln[0] and sorted(sum((g["params"] for g in g_ln), [])) == sorted(ln)
    # BERT: the same rule on its own layer names
    bert = ["bert.embeddings.linear_video.weight", "bert.embeddings.LayerNorm.weight", "bert.encoder.layer.0.output.LayerNorm.bias",
            "bert.encoder.layer.1.output.LayerNorm.weight", "bert.encoder.layer.2.attention.output.LayerNorm.weight",
            "cls.predictions.transform.LayerNorm.weight"]
    gb = PG.layerwise_groups(bert, 3, 0.5)
    sb = {n: g.get("lr_scale", 1.0) for g in gb for n in g["params"]}
    assert [sb[n] for n in bert] == [0.125, 0.125, 0.25, 0.5, 1.0, 1.0]
    assert {n for g in gb if g.get("weight_decay") == 0.0 for n in g["params"]} == set(bert[1:])


def test_lr_scale(PG):
    gs = [dict(lr=1e-3), dict(lr=5e-4), dict(lr=123.0, lr_scale=0.25)]  # (after construction torch has filled `lr` in everywhere)
    assert PG.learning_rates(gs) == [1e-3, 5e-4, 2.5e-4]
    gs[0]["lr"] = 2e-3  # what adjust_learning_rate writes
    assert PG.learning_rates(gs) == [2e-3, 5e-4, 5e-4]
    PG.check_groups([dict(params=[], lr=1e-3), dict(params=[], lr_scale=0.5)])
    with pytest.raises(ValueError, match="both"):
        PG.check_groups([dict(params=[]), dict(params=[], lr=1e-3, lr_scale=0.5)])
    with pytest.raises(ValueError, match="group 0"):
        PG.check_groups([dict(params=[], lr_scale=0.5)])
    with pytest.raises(ValueError, match="64"):
        PG.check_groups([dict(params=[])] * 65)


def test_state_dict_index_map(PG):
    members = PG.resolve([dict(params=[]), dict(params=["*LayerNorm*"]), dict(params=["*.bias"])],
                         [n for n in NAMES if not ("LayerNorm" in n and "bias" in n)])
    idx = PG.index_lists(members)
    assert [len(i) for i in idx] == [len(m) for m in members] and len(idx) == 3
    assert idx[0] == list(range(len(members[0])))
    assert idx[1] == list(range(len(members[0]), len(members[0]) + len(members[1])))
    assert idx[2][-1] == sum(len(m) for m in members) - 1 and idx[2][0] == idx[1][-1] + 1
    assert PG.index_lists([["a"], [], ["b", "c"]]) == [[0], [], [1, 2]]
