"""CPU: the packed-row layout of the BERT engine (bert_engine.bert_packing) on host tensors: plen[b] is the last position that
anything reads + 1, at least the video slots, at least 1 -- and the whole row for a sample without a valid key."""
import torch

from frozenbilm_amd.bert_engine import bert_packing


def _plen_ref(mask, labels, logit_rows, B, S, T):
    """the rules, spelled out position by position"""
    want = set(int(r) for r in logit_rows.view(-1)) if logit_rows is not None else set()
    out = []
    for b in range(B):
        last, any_valid = 0, False
        for s in range(S):
            valid = bool(mask[b * S + s] != 0)
            any_valid |= valid
            if valid or (labels is not None and int(labels[b * S + s]) != -100) or (b * S + s) in want:
                last = s + 1
        out.append(max(last, T, 1) if any_valid else S)
    return out


def _check(pk, plen, B, S):
    n = sum(plen)
    assert pk.n == n and pk.sel.numel() == n and pk.pos.numel() == n and pk.inv.numel() == B * S
    assert pk.row0.dtype == torch.int32 and pk.row0.tolist() == [sum(plen[:b]) for b in range(B + 1)]
    sel, pos = [], []
    for b in range(B):
        sel += [b * S + s for s in range(plen[b])]
        pos += list(range(plen[b]))
    assert pk.sel.tolist() == sel and pk.pos.tolist() == pos
    # sel, inv and pos are mutually consistent
    assert torch.equal(pk.inv[pk.sel], torch.arange(n))
    assert torch.equal(pk.sel % S, pk.pos)
    without = torch.ones(B * S, dtype=torch.bool)
    without[pk.sel] = False
    assert bool((pk.inv[without] == -1).all()) and int((pk.inv >= 0).sum()) == n


def _case(B=5, S=12, T=4):
    mask = torch.zeros(B, S, dtype=torch.int32)
    mask[0, :7] = 1
    mask[1, :5] = 1
    mask[1, 2] = 0           # a masked video slot inside [0, T)
    mask[2, :2] = 1          # shorter than the video slots: plen = T
    mask[3] = 0              # no valid key: the whole row
    mask[4, :9] = 1
    labels = torch.full((B, S), -100, dtype=torch.long)
    labels[0, 5] = 3
    labels[1, 8] = 7         # a label beyond the last valid token
    return mask.view(-1), labels.view(-1)


def test_plen_follows_the_rules_with_labels():
    B, S, T = 5, 12, 4
    mask, labels = _case(B, S, T)
    plen = _plen_ref(mask, labels, None, B, S, T)
    assert plen == [7, 9, 4, 12, 9]
    _check(bert_packing(mask, labels, None, B, S, T), plen, B, S)


def test_plen_follows_the_rules_with_logit_rows():
    B, S, T = 5, 12, 4
    mask, _ = _case(B, S, T)
    rows = torch.tensor([0 * S + 3, 4 * S + 10, 2 * S + 1])  # sample 4: a requested row beyond its last valid token
    plen = _plen_ref(mask, None, rows, B, S, T)
    assert plen == [7, 5, 4, 12, 11]
    _check(bert_packing(mask, None, rows, B, S, T), plen, B, S)
    # labels and logit rows together (the engine never passes both, the function does not care)
    _, labels = _case(B, S, T)
    plen = _plen_ref(mask, labels, rows, B, S, T)
    assert plen == [7, 9, 4, 12, 11]
    _check(bert_packing(mask, labels, rows, B, S, T), plen, B, S)


def test_text_only_batch_and_a_sample_without_a_valid_key():
    B, S, T = 4, 9, 0
    mask = torch.zeros(B, S, dtype=torch.int32)
    mask[0, :9] = 1
    mask[1, :1] = 1
    mask[2, 3] = 1   # zeros in front of the only valid token
    labels = torch.full((B, S), -100, dtype=torch.long)
    labels[1, 0] = 5
    plen = _plen_ref(mask.view(-1), labels.view(-1), None, B, S, T)
    assert plen == [9, 1, 4, 9]  # sample 3 has no valid key and keeps all S rows
    _check(bert_packing(mask.view(-1), labels.view(-1), None, B, S, T), plen, B, S)


def test_random_batches_against_the_loop():
    g = torch.Generator().manual_seed(3)
    for _ in range(20):
        B, S, T = int(torch.randint(1, 6, (1,), generator=g)), int(torch.randint(2, 20, (1,), generator=g)), 0
        T = int(torch.randint(0, min(S, 5), (1,), generator=g))
        lens = torch.randint(0, S + 1, (B,), generator=g)
        mask = (torch.arange(S)[None] < lens[:, None]).to(torch.int32)
        mask = mask * (torch.rand(B, S, generator=g) > 0.1).to(torch.int32)
        labels = torch.where(torch.rand(B, S, generator=g) < 0.05, torch.ones(B, S, dtype=torch.long), torch.full((B, S), -100))
        plen = _plen_ref(mask.view(-1), labels.view(-1), None, B, S, T)
        pk = bert_packing(mask.view(-1), labels.view(-1), None, B, S, T)
        if sum(plen) >= B * S:
            assert pk is None
        else:
            _check(pk, plen, B, S)


def test_a_full_batch_is_not_packed():
    B, S, T = 3, 8, 2
    mask = torch.ones(B * S, dtype=torch.int32)
    assert bert_packing(mask, None, torch.tensor([1]), B, S, T) is None
    # ... nor one whose only short sample has no valid key
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[1] = 0
    labels = torch.full((B * S,), -100, dtype=torch.long)
    assert bert_packing(mask.view(-1), labels, None, B, S, T) is None
