"""GPU: the BERT variant on packed rows (model.packed_rows, bert_engine.bert_packing) against the CPU oracle
oracle/bert_oracle.py and against the same model on the padded grid."""
import math

import pytest
import torch

from frozenbilm_amd.model import BertConfig, BertForMaskedLM
from oracle import bert_oracle as O
from tests.dropout_replay import attn_mask, row_mask
from tests.test_gpu_bert import SMALL, _batch, _check_grads, _masked_forward, _params, _rel, _to, _trainable

pytestmark = pytest.mark.gpu
DEV = "cuda"
# several key tiles and heads: S = 4 + 126 = 130 is three key tiles, the last one two rows wide
MULTI = dict(vocab_size=300, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
             max_position_embeddings=160)
CONFIGS = {"small": SMALL, "multi": MULTI}


def _ocfg(dims, n_ans=0):
    return O.BertOracleConfig(**dims, features_dim=32, max_feats=4, n_ans=n_ans)


def _model(dims, P, n_ans=0, p_hid=0.1, p_att=0.1, train=False):
    m = BertForMaskedLM(BertConfig(**dims, hidden_dropout_prob=p_hid, attention_probs_dropout_prob=p_att), features_dim=32,
                        max_feats=4, n_ans=n_ans)
    m.load_state_dict(P, strict=False)
    m.to(DEV)
    return m.train() if train else m.eval()


def _multi_batch(seed=5, V=300):
    """B = 4, T = 4, Lt = 126: text lengths [126, 60, 5, 0]; sample 3 has no valid key at all (its video mask is zero too),
    sample 1 a masked video slot; labels on every third valid token"""
    B, T, Lt = 4, 4, 126
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, T, 32, generator=g)
    vm = torch.ones(B, T, dtype=torch.long)
    vm[1, 2] = 0
    vm[3] = 0
    ids = torch.randint(5, V, (B, Lt), generator=g)
    am = torch.zeros(B, Lt, dtype=torch.long)
    for b, n in enumerate([126, 60, 5, 0]):
        am[b, :n] = 1
    ids[am == 0] = 0
    labels = torch.full((B, Lt), -100)
    labels[:, 1::3] = ids[:, 1::3]
    labels[am == 0] = -100
    return dict(video=video, video_mask=vm, input_ids=ids, attention_mask=am, labels=labels)


def _the_batch(name, seed=5):
    return _batch(seed=seed) if name == "small" else _multi_batch(seed=seed)


def _mask_rows(name):
    """one [MASK]-like grid row per sample (sample 3 of the multi-tile batch: a row of a sample without a valid key)"""
    S, text_pos = (16, [3, 10, 1]) if name == "small" else (130, [100, 30, 2, 0])
    return torch.tensor([b * S + 4 + t for b, t in enumerate(text_pos)])


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad}


def _worst_rel(a, b):
    return max((a[n] - b[n]).norm().item() / (b[n].norm().item() + 1e-12) for n in b)


def _packing_of(out, B, S):
    run = out.__dict__["_run"]
    assert run.pk is not None and run.N == run.pk.n < B * S, "the batch was not packed"
    have = torch.zeros(B * S, dtype=torch.bool, device=DEV)
    have[run.pk.sel] = True
    return run, have.view(B, S)


@pytest.mark.parametrize("name", ["small", "multi"])
def test_eval_with_labels_on_packed_rows(name):
    dims = CONFIGS[name]
    cfg = _ocfg(dims)
    P = _params(cfg)
    b = _the_batch(name)
    B, S = b["input_ids"].shape[0], b["input_ids"].shape[1] + 4
    _trainable(P)
    ref = O.forward(cfg, P, **b)
    ref["loss"].backward()
    m = _model(dims, P)
    m.packed_rows = True
    out = m(**_to(b), output_hidden_states=True)
    run, have = _packing_of(out, B, S)   # (fails where packed_rows is ignored)
    hv = have.cpu()
    logits = out.logits.detach().float().cpu()
    assert abs(out.loss.item() - ref["loss"].item()) < 2e-2
    assert (logits - ref["logits"].detach())[hv].abs().max().item() < 5e-2
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1
    assert (out.hidden_states[-1].cpu() - ref["hidden"].detach())[hv].abs().max().item() < 5e-2
    # positions without a row read as exactly zero
    assert not bool(hv.all())
    assert bool((logits[~hv] == 0).all()) and all(bool((h.cpu()[~hv] == 0).all()) for h in out.hidden_states)
    out.loss.backward()
    _check_grads(m, P)
    packed_loss, packed = out.loss.item(), _grads(m)
    # the same model on the padded grid
    m.packed_rows = False
    m.zero_grad(set_to_none=True)
    out = m(**_to(b))
    assert out.__dict__["_run"].pk is None
    out.loss.backward()
    worst = _worst_rel(packed, _grads(m))
    print(f"[bert packed {name}] rows {run.N} of {B * S}; packed vs padded: loss {abs(packed_loss - out.loss.item()):.3g}, "
          f"worst relative gradient difference {worst:.3g}")
    assert abs(packed_loss - out.loss.item()) < 1e-5
    assert worst < 1e-5
    # a loss on the logits back-propagates from the rows that exist
    w = torch.randn(ref["logits"].shape, generator=torch.Generator().manual_seed(2)) * hv[:, :, None]
    for v in P.values():
        v.grad = None
    (O.forward(cfg, P, **b)["logits"] * w).sum().div(100).backward()
    m.packed_rows = True
    m.zero_grad(set_to_none=True)
    out = m(**_to(b))
    _packing_of(out, B, S)
    (out.logits * w.to(DEV)).sum().div(100).backward()
    _check_grads(m, P)


@pytest.mark.parametrize("name", ["small", "multi"])
def test_logit_rows_inference_on_packed_rows(name):
    dims = CONFIGS[name]
    cfg = _ocfg(dims, n_ans=7)
    P = _params(cfg, seed=4)
    b = _the_batch(name, seed=7)
    b.pop("labels")
    B, S = b["input_ids"].shape[0], b["input_ids"].shape[1] + 4
    rows = _mask_rows(name).to(DEV)
    m = _model(dims, P, n_ans=7)
    with torch.no_grad():
        for mlm in (False, True):
            m.packed_rows = False
            want = m(**_to(b), logit_rows=rows, mlm=mlm).logits
            m.packed_rows = True
            out = m(**_to(b), logit_rows=rows, mlm=mlm)
            _packing_of(out, B, S)
            assert out.logits.shape == (rows.numel(), 300 if mlm else 7)
            r = (out.logits - want).norm().item() / want.norm().item()
            print(f"[bert packed {name}] logit_rows mlm={mlm}: relative difference {r:.3g}")
            assert r < 1e-5


@pytest.mark.parametrize("name", ["small", "multi"])
def test_train_mode_attention_dropout_does_not_depend_on_the_layout(name):
    """hidden dropout 0, attention dropout 0.1: the attention masks are keyed by (sample, head, query, key) positions"""
    dims = CONFIGS[name]
    cfg = _ocfg(dims)
    P = _params(cfg, seed=8)
    b = _the_batch(name, seed=9)
    B, S = b["input_ids"].shape[0], b["input_ids"].shape[1] + 4
    m = _model(dims, P, p_hid=0.0, p_att=0.1, train=True)
    res = {}
    for packed in (False, True):
        m.packed_rows = packed
        m.step_seed = 0  # both runs are the same step of the mask stream
        m.zero_grad(set_to_none=True)
        out = m(**_to(b))
        if packed:
            _packing_of(out, B, S)
        out.loss.backward()
        res[packed] = (out.loss.item(), _grads(m), [sv.seed_att for sv in out.__dict__["_run"].layers])
    assert res[True][2] == res[False][2] and all(res[True][2])
    m.eval()
    with torch.no_grad():
        assert abs(m(**_to(b)).loss.item() - res[True][0]) > 1e-4  # dropout made a difference
    worst = _worst_rel(res[True][1], res[False][1])
    print(f"[bert packed {name}] attention dropout, packed vs padded: loss {abs(res[True][0] - res[False][0]):.3g}, "
          f"worst relative gradient difference {worst:.3g}")
    assert abs(res[True][0] - res[False][0]) < 1e-5
    assert worst < 1e-5


@pytest.mark.parametrize("name", ["small", "multi"])
def test_train_mode_dropout_on_packed_rows_replays_into_the_oracle(name):
    dims = CONFIGS[name]
    cfg = _ocfg(dims)
    P = _params(cfg, seed=8)
    b = _the_batch(name, seed=9)
    B, S = b["input_ids"].shape[0], b["input_ids"].shape[1] + 4
    H, nh, p = dims["hidden_size"], dims["num_attention_heads"], 0.1
    _trainable(P)
    m = _model(dims, P, p_hid=p, p_att=p, train=True)
    m.packed_rows = True
    out = m(**_to(b))
    run, have = _packing_of(out, B, S)
    sel = run.pk.sel.cpu()

    def grid(seed):  # the row-wise sites are keyed by the packed element index; positions without a row: no dropout
        g = torch.ones(B * S, H)
        g[sel] = row_mask(seed, (run.N, H), p)
        return g

    masks = dict(emb=grid(run.seed_emb), att=[attn_mask(sv.seed_att, B, nh, S, p) for sv in run.layers],
                 ln1=[grid(sv.seed_ln1) for sv in run.layers], ln2=[grid(sv.seed_ln2) for sv in run.layers])
    loss_r, logits_r = _masked_forward(cfg, P, b, masks, p)
    hv = have.cpu()
    assert abs(out.loss.item() - loss_r.item()) < 2e-2
    assert (out.logits.detach().float().cpu() - logits_r.detach())[hv].abs().max().item() < 5e-2
    loss_r.backward()
    out.loss.backward()
    _check_grads(m, P)


def test_loops_run_on_packed_rows():
    from frozenbilm_amd import main as P_main
    from frozenbilm_amd import videoqa as P_vqa
    from frozenbilm_amd.optim import FusedAdam
    from tests.downstream_fixtures import Args, ListLoader, StubTokenizer, make_videoqa_batches, make_videotext_batches

    cfg = _ocfg(SMALL)
    P = _params(cfg, seed=12)
    tok, args = StubTokenizer(300), Args(max_feats=4, packed_rows=True)
    m = _model(SMALL, P)
    batches = make_videotext_batches(300, 4, 32, 2, 4, seed=31)
    tr = P_main.train_one_epoch(m, tok, ListLoader(batches), FusedAdam(m, lr=1e-3, betas=(0.9, 0.95)), torch.device(DEV), 0, args,
                                0.1)
    assert m.packed_rows and all(math.isfinite(v) for v in tr.values()), tr
    n_ans = 12
    Pa = _params(_ocfg(SMALL, n_ans=n_ans), seed=13)
    a2tok = torch.randint(1, 300, (n_ans, 2), generator=torch.Generator().manual_seed(1)).to(DEV)
    vb = make_videoqa_batches(300, 4, 32, n_ans, 2, 4, seed=41)
    preds = {}
    for packed in (False, True):
        m = _model(SMALL, Pa, n_ans=n_ans)
        m.set_answer_embeddings(a2tok)
        res, metrics = P_vqa.evaluate(m, tok, ListLoader(vb), torch.device(DEV), "msrvtt", Args(max_feats=4, packed_rows=packed),
                                      thresholds=[1, 10], split="test", type_map={0: "a", 1: "b"})
        assert m.packed_rows == packed and len(res) == 8 and all(math.isfinite(v) for v in metrics.values())
        preds[packed] = {q: r["pred"][0] for q, r in res.items()}
    assert preds[True] == preds[False]
