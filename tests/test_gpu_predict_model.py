"""GPU: `model.predict_topk` through both engines, every row layout, the launch-graph routes and the MLM loops.

Ids and ranks of two routes are compared exactly on the rows whose top-(k+1) logits are separated by more than SEP = 2e-3 (the
logit tolerance between two routes); a test may leave out at most 5 % of its rows for that (CAP).  The DeBERTa models use the
tiny configuration with synthetic parameters of std 0.2 (seed 74) and the BERT model the `SMALL` one (seed 2, std 0.2): their
logits have a standard deviation of ~2, and on the CPU oracles no labelled row of the batches below has two of its top six
logits within SEP (tests/test_predict_cases.py checks both); on the MI355X 1 of the 21 DeBERTa rows has.  Log-probabilities of
one layout are compared within the same SEP.

Measured on the MI355X, tiny DeBERTa, 6 seeds x std 0.05 / 0.1 / 0.2: the logits of one layout's loss rows and its filled logits
agree to ~3e-7, but the logits of two row LAYOUTS (grid, packed_rows, decoder_rows) differ by 3e-3 .. 7e-3 on the top six at
std 0.05 and 3e-2 .. 7e-2 at std 0.2 (bf16 activations rounded at other places) -- more than SEP.  The separation rule therefore
does not by itself make the ids of two layouts equal: at this seed they are (also at seed 78; at 75, 76, 77, 79 one to four
rows differ), and a label's rank is compared between layouts where the top-k ids decide it (the layout test labels each row
with one of the grid route's top five predictions)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from frozenbilm_amd import train_graph as TG  # noqa: E402
from oracle import bert_oracle as BO  # noqa: E402
from oracle import deberta_oracle as O  # noqa: E402
from tests import predict_cases as PC  # noqa: E402
from tests.downstream_fixtures import Args, ListLoader, StubTokenizer, make_videotext_batches  # noqa: E402
from tests.golden.make_goldens import _tiny_cfg, synth_batch  # noqa: E402
from tests.test_gpu_bert import SMALL, _batch as bert_batch, _model as bert_model, _to  # noqa: E402
from tests.test_gpu_model import build, to_dev  # noqa: E402

DEV = "cuda"
SEP, CAP, K = 2e-3, 0.05, 5
STD, SEED, BERT_SEED, BATCH = 0.2, 74, 2, dict(B=5, L=40, seed=31)  # (the same constants in tests/test_predict_cases.py)


def deberta(train=False, dropout=False):
    torch.manual_seed(0)
    cfg = _tiny_cfg()
    m = build(cfg, O.synth_params(cfg, seed=SEED, std=STD, ln_jitter=0.1), train=train)
    if not dropout:
        m.config.hidden_dropout_prob = m.config.attention_probs_dropout_prob = 0.0
        m.adapter_dropout = 0.0
    return cfg, m, to_dev(synth_batch(cfg, **BATCH))


def bert(train=False, dropout=False):
    torch.manual_seed(0)
    cfg = BO.BertOracleConfig(**SMALL, features_dim=32, max_feats=4, n_ans=0)
    m = bert_model(BO.synth_params(cfg, seed=BERT_SEED, std=STD, ln_jitter=0.1), p_drop=0.1 if dropout else 0.0, train=train)
    return cfg, m, _to(bert_batch())


MODELS = {"deberta": deberta, "bert": bert}


def grid_labels(batch, T):
    lab = batch["labels"]
    return torch.cat([torch.full((lab.shape[0], T), -100, device=lab.device), lab], 1).reshape(-1)


def separated(x, k=K):
    """bool [R]: the top-(k+1) logits of the row are pairwise more than SEP apart"""
    top = x.topk(min(k + 1, x.shape[1]), dim=1).values
    return ((top[:, :-1] - top[:, 1:]) > SEP).all(1)


def check_rows(p, batch, T):
    lab = grid_labels(batch, T)
    assert p.rows.dtype == torch.int64 and p.rows.numel() == p.rows.unique().numel()
    assert bool(((p.rows >= 0) & (p.rows < lab.numel())).all()) and bool((lab[p.rows] != -100).all())
    assert p.rows.numel() == int((lab != -100).sum()) and bool((p.rows[1:] > p.rows[:-1]).all())  # ascending grid index
    for t in (p.rows, p.topk_ids, p.topk_logprobs, p.label_rank, p.row_nll):
        assert not t.requires_grad and t.grad_fn is None
    assert p.topk_ids.dtype == torch.int64 and p.topk_ids.shape == p.topk_logprobs.shape == (p.rows.numel(), K)


def against_logits(what, p, x, labels=None):
    """predictions p against the reference applied to the logits x [R, V] of the same rows"""
    ref = PC.ref_predict(x, x.shape[1], K, labels)
    ok = separated(x)
    skipped = 1.0 - float(ok.float().mean())
    print(f"[predict model] {what}: {int((~ok).sum())} of {ok.numel()} rows not separated by {SEP}")
    assert skipped <= CAP, f"{what}: {skipped:.2%} of the rows are not separated"
    assert torch.equal(p.topk_ids[ok], ref["ids"][ok]), f"{what}: ids"
    d = (p.topk_logprobs.double() - ref["logprob"]).abs().max().item()
    print(f"[predict model] {what}: logprob max-abs diff {d:.3g}")
    assert d <= SEP, f"{what}: logprobs differ by {d}"
    if labels is not None:
        assert torch.equal(p.label_rank[ok], ref["rank"][ok]), f"{what}: ranks"
        dn = (p.row_nll.double() - ref["nll"]).abs().max().item()
        assert dn <= SEP, f"{what}: nll differs by {dn}"
    return ok


# ------------------------------------------------------------------------------------------------ 1. consistency, off by default
@pytest.mark.parametrize("packed", [False, True], ids=["grid", "packed"])
@pytest.mark.parametrize("name", ["deberta", "bert"])
def test_predictions_equal_the_reference_on_the_filled_logits(name, packed):
    cfg, m, batch = MODELS[name]()
    m.packed_rows = packed
    with torch.no_grad():
        off = m(**batch)
        assert m.predict_topk == 0 and off.predictions is None and off["predictions"] is None  # off by default
        m.predict_topk = K
        out = m(**batch)
        p = out.predictions
        assert p is out["predictions"] and p is not None
        run = out._run
        assert (run.pk is not None) == packed
        check_rows(p, batch, cfg.max_feats)
        assert torch.equal(out.loss, off.loss)
        # row_nll.mean() is the loss: the same R terms lse - x_label, summed in another order (R additions of fp32 rounding)
        R = p.rows.numel()
        assert abs(float(p.row_nll.double().mean()) - float(out.loss)) <= 2 * R * 2.0 ** -24 * float(p.row_nll.abs().max())
        assert run.logits_pending, "reading the predictions filled the [B*S, V] logits"
        m.predict_topk = 0
        second = m(**batch)  # an identical second call, whose logits are filled
        V = second.logits.shape[-1]
        x = second.logits.reshape(-1, V)[p.rows]
        assert run.logits_pending
    labels = grid_labels(batch, cfg.max_feats)[p.rows]
    against_logits(f"{name} packed={packed} labelled", p, x, labels)
    assert bool((p.correct(K) == (p.label_rank < K)).all()) and 0.0 <= float(p.accuracy()) <= float(p.accuracy(K)) <= 1.0


def test_validation_at_the_call():
    cfg, m, batch = deberta()
    for bad in (-1, 17, True, 2.0):
        m.predict_topk = bad
        with pytest.raises(ValueError):
            m(**batch)
    cfgb, mb, bb = bert()
    mb.predict_topk = 17
    with pytest.raises(ValueError):
        mb(**bb)


# ------------------------------------------------------------------------------------------------ 2. every layout
def test_same_answers_on_every_layout():
    cfg, m, batch = deberta()
    m.predict_topk = K
    T = cfg.max_feats
    got = {}
    with torch.no_grad():
        # every labelled position is labelled with one of the grid route's top five predictions for it (the forward does not
        # depend on the label values): ranks 0 .. 4, decided by the top-k ids
        first = m(**batch).predictions
        pick = first.topk_ids.gather(1, (torch.arange(first.rows.numel(), device=DEV) % K)[:, None])[:, 0]
        lab = grid_labels(batch, T)
        lab[first.rows] = pick
        batch = dict(batch, labels=lab.view(batch["labels"].shape[0], -1)[:, T:].contiguous())
        for packed, dec in ((False, False), (True, False), (False, True), (True, True)):
            m.packed_rows, m.decoder_rows = packed, dec
            out = m(**batch)
            assert (out._run.pk is not None) == packed and (out._run.dec_plan is not None) == dec
            check_rows(out.predictions, batch, T)
            got[(packed, dec)] = out.predictions
        m.packed_rows = m.decoder_rows = False
        m.predict_topk = 0
        ref_out = m(**batch)
        base = got[(False, False)]
        x = ref_out.logits.reshape(-1, ref_out.logits.shape[-1])[base.rows]
        ok = separated(x)
        assert 1.0 - float(ok.float().mean()) <= CAP
        m.predict_topk = K
        for layout, p in got.items():
            assert torch.equal(p.rows, base.rows), layout
            assert torch.equal(p.topk_ids[ok], base.topk_ids[ok]), f"{layout}: ids"
            assert torch.equal(p.label_rank[ok], base.label_rank[ok]), f"{layout}: ranks"
            assert torch.equal(base.label_rank[ok], (torch.arange(ok.numel(), device=DEV) % K)[ok])
            d = (p.topk_logprobs - base.topk_logprobs).abs().max().item()
            print(f"[predict model] layout packed, decoder_rows = {layout}: logprob max-abs diff to the grid {d:.3g}")
        # a logit_rows call on the labelled rows, in a shuffled order: the caller's order, no rank / NLL
        perm = torch.randperm(base.rows.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
        rows = base.rows[perm]
        feed = {k: v for k, v in batch.items() if k != "labels"}
        for packed, dec in ((False, False), (True, True)):
            m.packed_rows, m.decoder_rows = packed, dec
            out = m(**feed, logit_rows=rows, mlm=True)
            p = out.predictions
            assert torch.equal(p.rows, rows) and p.label_rank is None and p.row_nll is None
            assert torch.equal(p.topk_ids[ok[perm]], base.topk_ids[perm][ok[perm]]), f"logit_rows {packed, dec}: ids"
            against_logits(f"logit_rows packed={packed} decoder_rows={dec}", p, out.logits)
        # neither labels nor logit_rows: every grid row, from the logits the call returns
        m.packed_rows = m.decoder_rows = False
        out = m(**feed, mlm=True)
        p = out.predictions
        N = out.logits.shape[0] * out.logits.shape[1]
        assert torch.equal(p.rows, torch.arange(N, device=DEV)) and p.label_rank is None
        ref = PC.ref_predict(out.logits.reshape(N, -1), out.logits.shape[-1], K)
        assert torch.equal(p.topk_ids, ref["ids"])  # the same fp32 values: exact on every row
        assert torch.equal(p.topk_ids[base.rows][ok], base.topk_ids[ok])


def test_bert_same_answers_padded_and_packed():
    cfg, m, batch = bert()
    m.predict_topk = K
    got = {}
    with torch.no_grad():
        for packed in (False, True):
            m.packed_rows = packed
            out = m(**batch)
            assert (out._run.pk is not None) == packed
            got[packed] = out.predictions
        m.predict_topk, m.packed_rows = 0, False
        lg = m(**batch).logits
        ok = separated(lg.reshape(-1, lg.shape[-1])[got[False].rows])
    assert 1.0 - float(ok.float().mean()) <= CAP
    assert torch.equal(got[True].rows, got[False].rows)
    assert torch.equal(got[True].topk_ids[ok], got[False].topk_ids[ok]) and torch.equal(got[True].label_rank[ok], got[False].label_rank[ok])


def test_answer_head_uses_its_own_width():
    cfg = _tiny_cfg(n_ans=7)
    m = build(cfg, O.synth_params(cfg, seed=SEED, std=STD, ln_jitter=0.1))
    m.set_answer_embeddings(torch.randint(1, cfg.vocab_size, (7, 3), generator=torch.Generator().manual_seed(SEED)).to(DEV))
    batch = to_dev(synth_batch(cfg, **BATCH))
    feed = {k: v for k, v in batch.items() if k != "labels"}
    rows = torch.tensor([12, 70, 130], device=DEV)
    m.predict_topk = 16
    with torch.no_grad():
        out = m(**feed, logit_rows=rows)
    p = out.predictions
    assert out.logits.shape == (3, 7) and p.topk_ids.shape == (3, 16)
    ref = PC.ref_predict(out.logits, 7, 16)
    assert torch.equal(p.topk_ids, ref["ids"]) and bool((p.topk_ids[:, 7:] == -1).all())
    assert bool((p.topk_logprobs[:, 7:] == -float("inf")).all())


# ------------------------------------------------------------------------------------------------ 3. no effect on the step
@pytest.mark.parametrize("packed", [False, True], ids=["grid", "packed"])
@pytest.mark.parametrize("name", ["deberta", "bert"])
def test_a_training_step_is_bit_identical_with_and_without_predictions(name, packed):
    from frozenbilm_amd.optim import FusedAdam

    res = {}
    for k in (0, K):
        cfg, m, batch = MODELS[name](train=True, dropout=True)
        assert m.training and m.config.hidden_dropout_prob > 0
        m.packed_rows, m.predict_topk, m.step_seed = packed, k, 100
        opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
        out = m(**batch)
        assert (out.predictions is not None) == bool(k)
        if k:
            assert not out.predictions.topk_logprobs.requires_grad and not out.predictions.row_nll.requires_grad
        out.loss.backward()
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        opt.step(clip_max_norm=0.1)
        params = {n: p.detach().clone() for n, p in m.named_parameters()}
        res[k] = (out.loss.detach().clone(), grads, params)
    assert torch.equal(res[0][0], res[K][0]), "loss"
    assert res[0][1].keys() == res[K][1].keys() and len(res[0][1]) > 0
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[K][1][n]), f"grad of {n}"
    for n in res[0][2]:
        assert torch.equal(res[0][2][n], res[K][2][n]), f"parameter {n} after the step"


# ------------------------------------------------------------------------------------------------ 4. graph routes
def test_a_predict_topk_call_runs_eagerly_and_the_graph_route_serves_the_next():
    cfg, m, batch = deberta(train=True)
    m.training_graphs = True
    m.predict_topk = K
    out = m(**batch)
    out.loss.backward()
    st = TG.stats(m, TG.MLM)
    assert out.predictions is not None and st.captures == 0 and st.replays == 0 and not m.__dict__.get(TG.MLM.cache)
    m.predict_topk = 0
    for _ in range(3):
        o = m(**batch)
        assert o.predictions is None
        o.loss.backward()
    st = TG.stats(m, TG.MLM)
    assert st.captures == 1 and st.replays >= 1
    # the fine-tuning route (logit_rows under autograd)
    m.training_graphs, m.finetune_graphs = False, True
    feed = {k: v for k, v in batch.items() if k != "labels"}
    rows = torch.nonzero(grid_labels(batch, cfg.max_feats) != -100).view(-1)
    m.predict_topk = K
    o = m(**feed, logit_rows=rows, mlm=True)
    o.logits.float().sum().backward()
    st = TG.stats(m, TG.FINETUNE)
    assert o.predictions is not None and st.captures == 0 and st.replays == 0
    m.predict_topk = 0
    for _ in range(3):
        o = m(**feed, logit_rows=rows, mlm=True)
        o.logits.float().sum().backward()
    st = TG.stats(m, TG.FINETUNE)
    assert st.captures == 1 and st.replays >= 1


# ------------------------------------------------------------------------------------------------ 5. the MLM loops
def test_main_loops_log_mlm_accuracy():
    from frozenbilm_amd import main as P_main
    from frozenbilm_amd.optim import FusedAdam

    def fresh(train=False):
        cfg, m, _ = deberta(train=train)
        return cfg, m

    cfg, m = fresh()
    tok = StubTokenizer(cfg.vocab_size)
    batches = make_videotext_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, 3, 6, seed=31)
    dev = torch.device(DEV)
    plain, flagged = Args(max_feats=cfg.max_feats), Args(max_feats=cfg.max_feats)
    flagged.mlm_accuracy = True
    torch.manual_seed(7)
    base = P_main.evaluate(m, tok, ListLoader(batches), dev, plain)
    assert set(base) == {"loss", "mlm_loss"}  # without the flag: exactly today's keys
    torch.manual_seed(7)
    got = P_main.evaluate(m, tok, ListLoader(batches), dev, flagged)
    assert set(got) == {"loss", "mlm_loss", "mlm_acc", "mlm_acc5"} and m.predict_topk == 0
    assert got["loss"] == base["loss"] and got["mlm_loss"] == base["mlm_loss"]
    assert 0.0 <= got["mlm_acc"] <= got["mlm_acc5"] <= 1.0
    # recomputed from out.logits of the same batches (the same mask_tokens draws); a label whose logit is within 2 SEP of another
    # logit may rank either way between the two routes: the recomputation gives an interval, one point when there is none
    torch.manual_seed(7)
    lo, hi = {1: [], 5: []}, {1: [], 5: []}
    m.eval()
    with torch.no_grad():
        for b in batches:
            feed = P_main._prepare(b, tok, dev, plain)
            lg = m(**feed).logits
            lab = grid_labels(feed, cfg.max_feats)
            rows = torch.nonzero(lab != -100).view(-1)
            x = lg.reshape(-1, lg.shape[-1])[rows].double()
            xl = x.gather(1, lab[rows][:, None])
            most = (x > xl - 2 * SEP).sum(1) - 1  # every near-tie counted against the label (itself excluded)
            least = (x > xl + 2 * SEP).sum(1)
            for n in (1, 5):
                lo[n].append(float((most < n).double().mean()))
                hi[n].append(float((least < n).double().mean()))
    for n, key in ((1, "mlm_acc"), (5, "mlm_acc5")):
        a, b_ = sum(lo[n]) / len(lo[n]), sum(hi[n]) / len(hi[n])
        print(f"[predict model] evaluate {key} = {got[key]:.6f}, recomputed from out.logits in [{a:.6f}, {b_:.6f}]")
        assert a - 1e-6 <= got[key] <= b_ + 1e-6
    # training: the same losses as a run without the flag, the two meters next to them
    res = {}
    for name, args in (("plain", plain), ("flagged", flagged)):
        cfg, mt = fresh(train=True)
        torch.manual_seed(8)
        res[name] = P_main.train_one_epoch(mt, tok, ListLoader(batches), FusedAdam(mt, lr=1e-3, betas=(0.9, 0.95)), dev, 0, args, 0.1)
        assert mt.predict_topk == 0
    assert set(res["flagged"]) == set(res["plain"]) | {"mlm_acc", "mlm_acc5"} and "mlm_acc" not in res["plain"]
    assert res["flagged"]["loss"] == res["plain"]["loss"] and res["flagged"]["mlm_loss"] == res["plain"]["mlm_loss"]
    assert 0.0 <= res["flagged"]["mlm_acc"] <= res["flagged"]["mlm_acc5"] <= 1.0
