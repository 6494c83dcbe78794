"""Host logic of the fine-tuning rows route (videoqa.answer_logits, videoqa / mc train_one_epoch): which keyword arguments
the loops hand to a model that has an engine, with and without the opt-ins ``args.train_logit_rows`` / ``args.packed_rows``.
The model is a stub that records its calls; its logits are the same function of the grid row on both routes."""
import types

import pytest
import torch

from frozenbilm_amd import mc as P_mc
from frozenbilm_amd import videoqa as P_vqa
from frozenbilm_amd.engine import check_logit_rows
from frozenbilm_amd.loops import tokenize, video_inputs
from tests.downstream_fixtures import Args, ListLoader, StubTokenizer, make_mc_batches, make_videoqa_batches

VOCAB, T, F = 300, 4, 8


class StubModel(torch.nn.Module):
    """Looks like the MI355X model to the loops (``engine``, ``packed_rows``); logits[b*S + s, a] = w[a] * (1 + 0.01 * row)."""

    def __init__(self, n_ans):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(-1.0, 1.0, n_ans))
        self.packed_rows = False
        self.calls = []

    def engine(self):
        return types.SimpleNamespace(reducer=None)

    def forward(self, logit_rows=None, **feed):
        self.calls.append(dict(feed, logit_rows=logit_rows, grad=torch.is_grad_enabled(), packed_rows=self.packed_rows))
        B, Lt = feed["input_ids"].shape
        S = feed["video"].shape[1] + Lt
        grid = self.w[None] * (1 + 0.01 * torch.arange(B * S, dtype=torch.float32)[:, None])
        if logit_rows is not None:
            return {"logits": grid[logit_rows.long()]}
        return {"logits": grid.view(B, S, -1)}


class PlainModel(torch.nn.Module):
    """a model without an engine: its forward does not know ``logit_rows``"""

    def __init__(self, n_ans):
        super().__init__()
        self.n_ans, self.n_calls = n_ans, 0

    def forward(self, video, video_mask, input_ids, attention_mask):
        self.n_calls += 1
        return {"logits": torch.zeros(input_ids.shape[0], video.shape[1] + input_ids.shape[1], self.n_ans)}


def _feed(batch, tok, args):
    video, vmask = video_inputs(batch, torch.device("cpu"))
    enc = tokenize(tok, batch["text"], args)
    return enc, dict(video=video, video_mask=vmask, input_ids=enc["input_ids"], attention_mask=enc["attention_mask"])


@pytest.fixture()
def vqa_batch():
    return make_videoqa_batches(VOCAB, T, F, 6, 1, 5, seed=3)[0]


def test_without_the_opt_ins_a_training_pass_asks_for_the_full_logits(vqa_batch):
    tok, args, m = StubTokenizer(VOCAB), Args(max_feats=T), StubModel(6)
    enc, feed = _feed(vqa_batch, tok, args)
    out = P_vqa.answer_logits(m, tok, enc["input_ids"], args, **feed)
    assert m.calls[-1]["logit_rows"] is None and m.calls[-1]["grad"]
    assert out.shape == (5, 6) and out.requires_grad


@pytest.mark.parametrize("opt_in", ["train_logit_rows", "packed_rows"])
def test_with_an_opt_in_a_training_pass_hands_over_the_mask_rows(vqa_batch, opt_in):
    tok, m = StubTokenizer(VOCAB), StubModel(6)
    args = Args(max_feats=T, **{opt_in: True})
    enc, feed = _feed(vqa_batch, tok, args)
    full = P_vqa.answer_logits(m, tok, enc["input_ids"], Args(max_feats=T), **feed)
    out = P_vqa.answer_logits(m, tok, enc["input_ids"], args, **feed)
    rows = m.calls[-1]["logit_rows"]
    assert rows is not None and m.calls[-1]["grad"]
    assert torch.equal(rows, P_vqa.mask_rows(enc["input_ids"], tok, args, torch.device("cpu")))
    assert out.requires_grad and torch.equal(out, full)  # the rows mask_row_logits reads, in its order


def test_under_no_grad_the_rows_route_is_taken_whatever_args_say(vqa_batch):
    tok, m = StubTokenizer(VOCAB), StubModel(6)
    for args in (Args(max_feats=T), Args(max_feats=T, train_logit_rows=True)):
        enc, feed = _feed(vqa_batch, tok, args)
        with torch.no_grad():
            P_vqa.answer_logits(m, tok, enc["input_ids"], args, **feed)
        assert m.calls[-1]["logit_rows"] is not None and not m.calls[-1]["grad"]
    # a model without an engine (the CPU oracle, the reference) never sees the keyword, opt-in or not
    plain = PlainModel(6)
    args = Args(max_feats=T, train_logit_rows=True, packed_rows=True)
    enc, feed = _feed(vqa_batch, tok, args)
    out = P_vqa.answer_logits(plain, tok, enc["input_ids"], args, **feed)
    assert out.shape == (5, 6) and plain.n_calls == 1


@pytest.mark.parametrize("packed", [False, True])
def test_videoqa_training_loop_follows_args_packed_rows(packed):
    tok, m = StubTokenizer(VOCAB), StubModel(6)
    args = Args(max_feats=T, packed_rows=packed)
    batches = make_videoqa_batches(VOCAB, T, F, 6, 2, 4, seed=5)
    w0 = m.w.detach().clone()
    stats = P_vqa.train_one_epoch(m, tok, ListLoader(batches), torch.optim.SGD(m.parameters(), lr=0.1), torch.device("cpu"), 0,
                                  "msrvtt", args)
    assert m.packed_rows is packed and m.training
    assert len(m.calls) == 2 and all(c["grad"] and c["packed_rows"] is packed for c in m.calls)
    assert all((c["logit_rows"] is not None) == packed for c in m.calls)
    for c, b in zip(m.calls, batches):  # the inputs of the training loop: the tokenizer's, the separator token left alone
        enc = tokenize(tok, b["text"], args)
        assert torch.equal(c["input_ids"], enc["input_ids"]) and torch.equal(c["attention_mask"], enc["attention_mask"])
    assert "cls_loss" in stats and not torch.equal(m.w.detach(), w0)


@pytest.mark.parametrize("packed,sequential", [(False, False), (True, False), (True, True)])
def test_mc_training_loop_follows_args_packed_rows(packed, sequential):
    tok, m = StubTokenizer(VOCAB), StubModel(2)
    args = Args(max_feats=T, packed_rows=packed, mc_sequential=sequential)
    batches = make_mc_batches(VOCAB, T, F, 4, 2, 3, seed=7)
    stats = P_mc.train_one_epoch(m, tok, ListLoader(batches, mc=4), torch.optim.SGD(m.parameters(), lr=0.1), torch.device("cpu"),
                                 0, args)
    assert m.packed_rows is packed
    assert len(m.calls) == (8 if sequential else 2)  # one forward per candidate, or one per batch
    assert all((c["logit_rows"] is not None) == packed and c["grad"] for c in m.calls)
    if packed:  # one [MASK] row per text of the forward
        assert all(c["logit_rows"].numel() == c["input_ids"].shape[0] for c in m.calls)
    assert "cls_loss" in stats


def test_check_logit_rows():
    check_logit_rows(torch.tensor([], dtype=torch.long), 10)
    check_logit_rows(torch.tensor([9, 0, 4]), 10)
    check_logit_rows(torch.tensor([3], dtype=torch.int32), 10)
    for bad in ([10], [-1, 2], [0, 11, 3]):
        with pytest.raises(ValueError, match="token grid"):
            check_logit_rows(torch.tensor(bad), 10)
    with pytest.raises(ValueError, match="more than once"):
        check_logit_rows(torch.tensor([4, 1, 4]), 10)
