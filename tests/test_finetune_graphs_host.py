"""Host logic of the fine-tuning launch graphs (``model.finetune_graphs`` / ``args.finetune_graphs``): the length bucket and
the row remap of the padded batch, the attribute on both models, and what the two training loops do with the argument.
The loops run against the recording stub of test_finetune_rows_host."""
import warnings

import pytest
import torch

from frozenbilm_amd import mc as P_mc
from frozenbilm_amd import videoqa as P_vqa
from frozenbilm_amd.model import DebertaV2Config, DebertaV2ForMaskedLM
from frozenbilm_amd.train_graph import bucket_length, remap_rows
from tests.downstream_fixtures import Args, ListLoader, StubTokenizer, make_mc_batches, make_videoqa_batches
from tests.test_bert_host import _small
from tests.test_finetune_rows_host import F, T, VOCAB, PlainModel, StubModel, _feed

BUCKET = DebertaV2ForMaskedLM.GRAPH_L_BUCKET


# ------------------------------------------------------------------------------------------------ the bucket helper
@pytest.mark.parametrize("Lt,Lp", [(1, 32), (31, 32), (32, 32), (33, 64), (64, 64)])
def test_text_is_padded_to_the_next_multiple_of_the_bucket(Lt, Lp):
    assert BUCKET == 32
    assert bucket_length(Lt, 10, 512, BUCKET) == Lp


def test_the_bucket_is_capped_by_the_position_table():
    assert bucket_length(500, 10, 512, BUCKET) == 502
    assert bucket_length(502, 10, 512, BUCKET) == 502
    assert bucket_length(503, 10, 512, BUCKET) is None  # the cap cuts below Lt: the eager path raises the reference's error
    assert bucket_length(40, 0, 32, BUCKET) is None


def test_rows_are_remapped_onto_the_padded_grid():
    Tv, Lt, Lp, B = 10, 21, 32, 4
    S_old, S_new = Tv + Lt, Tv + Lp
    cases = [(0, 0), (0, Tv - 1),           # video slots of the first sample
             (1, Tv), (2, Tv + 7),          # text
             (B - 1, 3), (B - 1, S_old - 1)]  # the last sample: a video slot, its last text position
    rows = torch.tensor([b * S_old + s for b, s in cases])
    got = remap_rows(rows, S_old, S_new)
    assert got.tolist() == [b * S_new + s for b, s in cases]
    assert int(got.max()) < B * S_new
    assert torch.equal(remap_rows(rows, S_old, S_old), rows)  # nothing padded: nothing moves
    # what the rows select is what they selected before: token (b, s) of the grid padded behind every sample
    grid = torch.arange(B * S_old).view(B, S_old)
    padded = torch.nn.functional.pad(grid, (0, Lp - Lt), value=-1)
    assert torch.equal(padded.reshape(-1)[got], grid.reshape(-1)[rows])


# ------------------------------------------------------------------------------------------------ the attribute
def test_deberta_model_has_the_switch_off_by_default():
    cfg = DebertaV2Config(vocab_size=128, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128)
    m = DebertaV2ForMaskedLM(cfg, max_feats=4, features_dim=32)
    assert m.finetune_graphs is False and m.training_graphs is False and m.inference_graphs is False
    m.finetune_graphs = True
    m.__dict__["_finetune_graph_cache"] = {"stale": object()}
    m.invalidate()  # an engine rebuild drops the captured steps of this route as well
    assert "_finetune_graph_cache" not in m.__dict__ and m.finetune_graphs is True


def test_bert_model_accepts_the_switch_and_ignores_it():
    m = _small()
    assert m.finetune_graphs is False
    m.packed_rows = m.inference_graphs = m.training_graphs = m.finetune_graphs = True
    assert m.step_seed == 0 and m._reducer is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (the call reaches the engine as it does without the switch)
        m(input_ids=torch.ones(2, 5, dtype=torch.long), logit_rows=torch.tensor([1, 6]))


# ------------------------------------------------------------------------------------------------ the loops
class GraphStub(StubModel):
    def __init__(self, n_ans):
        super().__init__(n_ans)
        self.finetune_graphs = False

    def forward(self, logit_rows=None, **feed):
        out = super().forward(logit_rows=logit_rows, **feed)
        self.calls[-1]["finetune_graphs"] = self.finetune_graphs
        return out


def test_the_argument_implies_the_rows_route():
    tok, m = StubTokenizer(VOCAB), StubModel(6)
    batch = make_videoqa_batches(VOCAB, T, F, 6, 1, 5, seed=3)[0]
    args = Args(max_feats=T, finetune_graphs=True)
    enc, feed = _feed(batch, tok, args)
    full = P_vqa.answer_logits(m, tok, enc["input_ids"], Args(max_feats=T), **feed)
    assert m.calls[-1]["logit_rows"] is None
    out = P_vqa.answer_logits(m, tok, enc["input_ids"], args, **feed)
    rows = m.calls[-1]["logit_rows"]
    assert rows is not None and m.calls[-1]["grad"]
    assert torch.equal(rows, P_vqa.mask_rows(enc["input_ids"], tok, args, torch.device("cpu")))
    assert out.requires_grad and torch.equal(out, full)
    plain = PlainModel(6)  # a model without an engine never sees the keyword
    assert P_vqa.answer_logits(plain, tok, enc["input_ids"], args, **feed).shape == (5, 6) and plain.n_calls == 1


@pytest.mark.parametrize("on", [False, True])
def test_videoqa_training_loop_follows_args_finetune_graphs(on):
    tok, m = StubTokenizer(VOCAB), GraphStub(6)
    args = Args(max_feats=T, finetune_graphs=on)
    batches = make_videoqa_batches(VOCAB, T, F, 6, 2, 4, seed=5)
    P_vqa.train_one_epoch(m, tok, ListLoader(batches), torch.optim.SGD(m.parameters(), lr=0.1), torch.device("cpu"), 0,
                          "msrvtt", args)
    assert m.finetune_graphs is on and m.packed_rows is False
    assert len(m.calls) == 2 and all(c["finetune_graphs"] is on and (c["logit_rows"] is not None) == on for c in m.calls)


def test_the_loops_set_the_switch_only_on_a_model_that_has_it():
    tok, args = StubTokenizer(VOCAB), Args(max_feats=T, finetune_graphs=True)
    m = StubModel(6)  # has an engine, lacks the attribute
    P_vqa.train_one_epoch(m, tok, ListLoader(make_videoqa_batches(VOCAB, T, F, 6, 1, 4, seed=5)),
                          torch.optim.SGD(m.parameters(), lr=0.1), torch.device("cpu"), 0, "msrvtt", args)
    assert not hasattr(m, "finetune_graphs") and m.calls[-1]["logit_rows"] is not None
    m2 = StubModel(2)
    P_mc.train_one_epoch(m2, tok, ListLoader(make_mc_batches(VOCAB, T, F, 4, 1, 3, seed=7), mc=4),
                         torch.optim.SGD(m2.parameters(), lr=0.1), torch.device("cpu"), 0, args)
    assert not hasattr(m2, "finetune_graphs")


@pytest.mark.parametrize("sequential", [False, True])
def test_mc_training_loop_leaves_the_switch_off_for_mc_sequential(sequential):
    tok, m = StubTokenizer(VOCAB), GraphStub(2)
    args = Args(max_feats=T, finetune_graphs=True, mc_sequential=sequential)
    batches = make_mc_batches(VOCAB, T, F, 4, 2, 3, seed=7)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        stats = P_mc.train_one_epoch(m, tok, ListLoader(batches, mc=4), torch.optim.SGD(m.parameters(), lr=0.1),
                                     torch.device("cpu"), 0, args)
    said = [w for w in seen if "mc_sequential" in str(w.message)]
    assert m.finetune_graphs is (not sequential)
    assert len(said) == (1 if sequential else 0)  # once per epoch call, not per step
    assert len(m.calls) == (8 if sequential else 2)
    assert all(c["logit_rows"] is not None and c["finetune_graphs"] is (not sequential) for c in m.calls)  # the rows route either way
    assert "cls_loss" in stats
