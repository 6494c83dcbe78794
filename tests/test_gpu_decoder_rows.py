"""GPU: the enhanced mask decoder on the selected rows only (opt-in ``model.decoder_rows``) against the full decoder, the CPU
oracle (eval mode, and train mode with the dropout masks replayed) and the recorded G10 / G11 / G13 loops.  Models are built as tests/test_gpu_finetune_rows.py builds them (the tiny
configuration of tests/golden/make_goldens._tiny_cfg); the bounds are those of the existing tests of the same comparisons:
loss / row logits 2e-2 and gradients 3e-2 relative Frobenius between two routes (test_packed_rows_route_equals_the_padded_rows_route),
the oracle bounds of test_gradient_through_the_rows_route_packed_vs_oracle, the loop bounds of test_videoqa_train_loop_on_packed_rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from frozenbilm_amd import mc as P_mc  # noqa: E402
from frozenbilm_amd import videoqa as P_vqa  # noqa: E402
from oracle.model_wrapper import OracleModel  # noqa: E402
from tests.downstream_fixtures import Args, ListLoader, StubTokenizer, make_mc_batches, make_videoqa_batches  # noqa: E402
from tests.golden.make_goldens import _tiny_cfg, synth_batch  # noqa: E402
from tests.test_downstream_loops import DELTA_KEYS, N_ANS, _j, cosine, tiny  # noqa: E402
from tests.test_gpu_downstream import hip_model  # noqa: E402
from tests.test_gpu_finetune_rows import _forward_at, _grads, _live_model, _ragged, _vqa_feed, _worst_rel  # noqa: E402
from oracle import deberta_oracle as O  # noqa: E402
from tests.test_gpu_model import build, to_dev  # noqa: E402

DEV = "cuda"


def _saved_rows(run):
    """the two decoder executions are the last two saved ones: the row count of what they kept"""
    assert all(sv.kvp is not None for sv in run.layers[-2:])
    return [sv.ctx.shape[0] for sv in run.layers[-2:]], [sv.ln2.t.shape[0] for sv in run.layers[-2:]]


def _mlm_model(train):
    """the tiny masked-LM model (vocabulary head); train: train mode with every dropout probability 0"""
    cfg = _tiny_cfg()
    m = build(cfg, O.synth_params(cfg, seed=74, std=0.05, ln_jitter=0.1), train=train)
    m.config.hidden_dropout_prob = m.config.attention_probs_dropout_prob = 0.0
    m.adapter_dropout = 0.0
    return cfg, m


def _labelled(cfg, B, Lt, seed):
    batch = synth_batch(cfg, B=B, L=Lt, seed=seed)
    assert (batch["labels"] != -100).sum() > 0
    return to_dev(batch)


# ------------------------------------------------------------------------------------------------ 1. on against off
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train_p0"])
@pytest.mark.parametrize("packed", [False, True], ids=["grid", "packed"])
def test_labelled_call_on_against_off(train, packed):
    cfg, m = _mlm_model(train)
    batch = _labelled(cfg, 5, 40, seed=31)
    R = int((batch["labels"] != -100).sum())
    res = {}
    for on in (False, True):
        m.packed_rows, m.decoder_rows = packed, on
        m.zero_grad(set_to_none=True)
        out = m(**batch)
        run = out._run
        assert (run.pk is not None) == packed and run.N == (run.pk.n if packed else 5 * run.S)  # run.N is unchanged
        if on:
            assert _saved_rows(run) == ([R, R], [R, R])
        out.loss.backward()
        res[on] = (out.loss.detach().clone(), _grads(m), out.logits.detach().clone(), run)
    d = (res[True][0] - res[False][0]).abs().item()
    worst = _worst_rel(res[True][1], res[False][1])
    print(f"[labelled on vs off train={train} packed={packed}] R={R} loss diff {d:.3g}, worst gradient Frobenius diff {worst:.3g}")
    assert d < 2e-2 and worst < 3e-2
    # out.logits: the selected rows, zero elsewhere
    lab = torch.cat([torch.full((5, cfg.max_feats), -100, device=DEV), batch["labels"]], 1) != -100
    lo_on, lo_off = res[True][2], res[False][2]
    assert (lo_on[~lab] == 0).all() and (lo_on[lab] - lo_off[lab]).abs().max().item() < 5e-2


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train_p0"])
def test_videoqa_rows_call_on_against_off(golden, train):
    g = golden("G10_videoqa", raw=True)
    cfg, P, m = hip_model(N_ANS, 10, g["a2tok"], train=train)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats)
    b, enc, feed = _vqa_feed(cfg, tok, args, 6, seed=77)
    rows = P_vqa.mask_rows(enc["input_ids"], tok, args, DEV)
    ans = b["answer_id"].to(DEV)
    res = {}
    for on in (False, True):
        m.decoder_rows = on
        m.zero_grad(set_to_none=True)
        out = m(**feed, logit_rows=rows)
        assert out["logits"].shape == (6, N_ANS) and out._run.N == 6 * out._run.S
        if on:
            assert _saved_rows(out._run) == ([6, 6], [6, 6])
        P_vqa.vqa_loss(out["logits"], ans, "msrvtt").backward()
        res[on] = (out["logits"].detach().clone(), _grads(m))
    d = (res[True][0] - res[False][0]).abs().max().item()
    worst = _worst_rel(res[True][1], res[False][1])
    print(f"[videoqa rows on vs off train={train}] logits max-abs diff {d:.3g}, worst gradient Frobenius diff {worst:.3g}")
    assert d < 2e-2 and worst < 3e-2


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train_p0"])
@pytest.mark.parametrize("B,Lt", [(5, 40), (3, 100), (4, 130)])  # S = 50, 110, 140
def test_rows_call_on_against_off_with_packed_rows(B, Lt, train):
    cfg = _tiny_cfg(n_ans=N_ANS)
    m = _live_model(cfg, 72, train=train)
    m.config.hidden_dropout_prob = m.config.attention_probs_dropout_prob = 0.0  # train mode with p = 0
    m.adapter_dropout = 0.0
    m.packed_rows = True
    feed, rows, ans, S = _ragged(cfg, B, Lt, seed=B + Lt)
    res = {}
    for on in (False, True):
        m.decoder_rows = on
        m.zero_grad(set_to_none=True)
        out = m(**feed, logit_rows=rows)
        assert out._run.pk is not None and out._run.N == out._run.pk.n < B * S and out._run.train == train and out._run.p_hid == 0
        P_vqa.vqa_loss(out["logits"], ans, "msrvtt").backward()
        res[on] = (out["logits"].detach().clone(), _grads(m))
    d = (res[True][0] - res[False][0]).abs().max().item()
    worst = _worst_rel(res[True][1], res[False][1])
    print(f"[rows packed on vs off S={S} train={train}] logits max-abs diff {d:.3g}, worst gradient Frobenius diff {worst:.3g}")
    assert d < 2e-2 and worst < 3e-2


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train_p0"])
def test_mc_candidate_scores_on_against_off(golden, train):
    g = golden("G11_mc", raw=True)
    cfg, P, m = hip_model(2, 11, g["a2tok"], train=train)  # (train: every dropout probability is 0)
    tok = StubTokenizer(cfg.vocab_size)
    b = make_mc_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, 4, 1, 5, seed=211, min_tok=4, max_tok=40)[0]
    gt = b["answer_id"].to(DEV)
    res = {}
    for on in (False, True):
        args = Args(max_feats=cfg.max_feats, train_logit_rows=True)
        m.decoder_rows = on
        m.zero_grad(set_to_none=True)
        scores = P_mc.candidate_scores(m, tok, b, torch.device(DEV), args)
        assert scores.shape == (5, 4) and scores.requires_grad
        P_mc.mc_loss(scores, gt, 4).backward()
        res[on] = (scores.detach().clone(), _grads(m))
    d = (res[True][0] - res[False][0]).abs().max().item()
    worst = _worst_rel(res[True][1], res[False][1])
    print(f"[mc on vs off train={train}] scores max-abs diff {d:.3g}, worst gradient Frobenius diff {worst:.3g}")
    assert d < 2e-2 and worst < 3e-2


# ------------------------------------------------------------------------------------------------ 2. against the oracle
def test_videoqa_rows_call_against_the_oracle(golden):
    g = golden("G10_videoqa", raw=True)
    cfg, P, m = hip_model(N_ANS, 10, g["a2tok"])
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats)
    b, enc, feed = _vqa_feed(cfg, tok, args, 6, seed=77)
    from frozenbilm_amd.util.misc import get_mask

    om = OracleModel(tiny(N_ANS), P, torch.as_tensor(g["a2tok"]))
    lo = P_vqa.mask_row_logits(om(video=b["video"], video_mask=get_mask(b["video_len"], cfg.max_feats), input_ids=enc["input_ids"],
                                  attention_mask=enc["attention_mask"])["logits"], enc["input_ids"], tok, args)
    loss_o = P_vqa.vqa_loss(lo, b["answer_id"], "msrvtt")
    loss_o.backward()
    m.decoder_rows = True
    out = m(**feed, logit_rows=P_vqa.mask_rows(enc["input_ids"], tok, args, DEV))
    assert out._run.dec_plan is not None
    assert (out["logits"].detach().cpu() - lo.detach()).abs().max().item() < 5e-2
    loss = P_vqa.vqa_loss(out["logits"], b["answer_id"].to(DEV), "msrvtt")
    print(f"[decoder rows vs oracle] loss {loss.item():.5f} vs {loss_o.item():.5f}")
    assert abs(loss.item() - loss_o.item()) < 2e-2
    loss.backward()
    ref = {n: p.grad for n, p in om.named_ref_parameters().items() if p.requires_grad}
    bad, worst = [], 0.0
    for name, p in m.named_parameters():
        if p.requires_grad:
            r = ref[name]
            rel = (p.grad.cpu() - r).norm().item() / (r.norm().item() + 1e-12)
            worst = max(worst, rel)
            if rel > (0.25 if "adapter.down" in name else 6e-2):
                bad.append((name, rel))
    print(f"[decoder rows vs oracle] worst gradient Frobenius diff {worst:.3g}")
    assert not bad, bad[:8]


def test_labelled_call_against_the_oracle_on_g5_inputs(golden):
    """the labelled call on G5's inputs against the reference's recorded loss, selected-row logits and gradients (the bounds of
    test_tiny_forward_golden / test_tiny_backward_golden)"""
    g = golden("G5_tiny_model")
    cfg = _tiny_cfg()
    m = build(cfg, O.synth_params(cfg, seed=5, std=0.05, ln_jitter=0.1))
    m.decoder_rows = True
    batch = {k[3:]: v for k, v in g.items() if k.startswith("in.")}
    out = m(**to_dev(batch))
    pl = out._run.dec_plan
    assert pl is not None and pl.R == int((batch["labels"] != -100).sum())
    assert abs(out.loss.item() - g["loss"].item()) < 2e-2
    sel = pl.grid.cpu()
    V = g["logits"].shape[-1]
    assert (out.logits.float().cpu().reshape(-1, V)[sel] - g["logits"].reshape(-1, V)[sel]).abs().max().item() < 5e-2
    out.loss.backward()
    bad = []
    for name, p in m.named_parameters():
        if p.requires_grad:
            ref = g["grad." + name]
            fro = (p.grad.float().cpu() - ref).norm().item() / max(ref.norm().item(), 1e-9)
            if fro > (0.25 if "adapter.down" in name else 6e-2):
                bad.append((name, round(fro, 4)))
    assert not bad, bad


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train_p0"])
def test_gradient_through_the_logits_of_a_labelled_call_on_against_off(train):
    """a labelled call returns differentiable logits next to its loss: a caller's extra term on them (here on the labelled rows,
    the rows that mean the same on both routes) flows back through the head and the decoder"""
    cfg, m = _mlm_model(train)
    batch = _labelled(cfg, 5, 40, seed=33)
    lab = torch.cat([torch.full((5, cfg.max_feats), -100, device=DEV), batch["labels"]], 1).view(-1) != -100
    res = {}
    for on in (False, True):
        m.decoder_rows = on
        m.zero_grad(set_to_none=True)
        out = m(**batch)
        assert (out._run.dec_plan is not None) == on
        lg = out.logits.reshape(lab.numel(), -1)
        extra = lg[lab].float().pow(2).mean()
        (out.loss + 0.5 * extra).backward()
        res[on] = (extra.detach().clone(), _grads(m))
        # a gradient handed in off the selected rows has nothing to flow into on the option-on route: it must not fault
        m.zero_grad(set_to_none=True)
        out = m(**batch)
        out.logits.float().sum().backward()
        assert all(torch.isfinite(v).all() for v in _grads(m).values())
    d = (res[True][0] - res[False][0]).abs().item()
    worst = _worst_rel(res[True][1], res[False][1])
    print(f"[through the logits of a labelled call, train={train}] extra term diff {d:.3g}, worst gradient Frobenius diff {worst:.3g}")
    assert d < 2e-2 and worst < 3e-2


def test_nothing_selected_under_gradients():
    """R = 0 with gradients: every label -100.  No decoder work, the backward runs through the encoder on zeros: every gradient is
    exactly zero and finite, as with the option off; the position chain keeps one entry per layer execution."""
    cfg, m = _mlm_model(True)
    batch = _labelled(cfg, 4, 40, seed=35)
    batch["labels"] = torch.full_like(batch["labels"], -100)
    res = {}
    for on in (False, True):
        m.decoder_rows = on
        m.zero_grad(set_to_none=True)
        out = m(**batch)
        assert (out._run.dec_plan is not None) == on and (not on or out._run.dec_plan.R == 0)
        assert torch.isnan(out.loss)  # the mean over no rows, on both routes
        out.loss.backward()
        res[on] = _grads(m)
    assert res[True].keys() == res[False].keys()
    for n in res[False]:
        assert torch.equal(res[True][n], torch.zeros_like(res[True][n])) and torch.equal(res[False][n], res[True][n]), n


def test_nothing_selected_with_live_dropout_draws_the_seeds_of_the_full_decoder():
    """R = 0 in train mode with every dropout probability at its configured non-zero value: the decoder that is not executed
    draws the seeds of all its sites, so the forward ends at the same place of the mask stream with the option on and off"""
    cfg = _tiny_cfg()
    m = build(cfg, O.synth_params(cfg, seed=74, std=0.05, ln_jitter=0.1), train=True)
    batch = _labelled(cfg, 4, 40, seed=35)
    batch["labels"] = torch.full_like(batch["labels"], -100)
    sites = {}
    for on in (False, True):
        m.decoder_rows = on
        run = _forward_at(m, batch, None, step_seed=3)._run
        assert run.p_hid > 0 and run.p_att > 0 and run.p_ad > 0
        assert (run.dec_plan is not None) == on and (not on or run.dec_plan.R == 0)
        sites[on] = run._site
    assert sites[True] == sites[False] > 0, sites


# ------------------------------------------------------------------------------------------------ 3. edges
def test_two_identically_seeded_training_steps_are_bit_identical():
    cfg = _tiny_cfg(n_ans=N_ANS)
    m = _live_model(cfg, 73, train=True)
    m.decoder_rows = True
    feed, rows, ans, S = _ragged(cfg, 6, 77, seed=9)
    got = []
    for _ in range(2):
        out = _forward_at(m, feed, rows, step_seed=3)
        assert out._run.dec_plan is not None and out._run.p_hid > 0 and out._run.p_att > 0
        loss = P_vqa.vqa_loss(out["logits"], ans, "msrvtt")
        loss.backward()
        flat = torch.cat([p.grad.reshape(-1) for p in m.parameters() if p.requires_grad]).clone()
        assert torch.isfinite(flat).all() and torch.isfinite(loss) and flat.abs().max().item() > 0
        got.append((out["logits"].detach().clone(), flat))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    # the option on and off draw the same number of seeds: the step after is at the same place of the mask stream
    sites = out._run._site
    m.decoder_rows = False
    assert _forward_at(m, feed, rows, step_seed=3)._run._site == sites


def test_edges_and_fallbacks(golden):
    g = golden("G10_videoqa", raw=True)
    cfg, P, m = hip_model(N_ANS, 10, g["a2tok"])
    cfg2, P2, never = hip_model(N_ANS, 10, g["a2tok"])  # a model that never had the attribute set
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats)
    b, enc, feed = _vqa_feed(cfg, tok, args, 4, seed=81)
    rows = P_vqa.mask_rows(enc["input_ids"], tok, args, DEV)
    with torch.no_grad():
        ref = never(**feed, logit_rows=rows)["logits"]
        ref_full = never(**feed)["logits"]
        m.decoder_rows = True
        on = m(**feed, logit_rows=rows)["logits"]
        assert (on - ref).abs().max().item() < 2e-2
        # duplicates without gradients: repeated rows, bit-equal; a shuffled list keeps the caller's order
        dup = torch.cat([rows, rows[:1]])
        a = m(**feed, logit_rows=dup)["logits"]
        assert a.shape == (5, N_ANS) and torch.equal(a[4], a[0]) and torch.equal(a[:4], on)
        perm = torch.tensor([2, 0, 3, 1], device=DEV)
        assert torch.equal(m(**feed, logit_rows=rows[perm])["logits"], on[perm])
        # R = 0
        empty = m(**feed, logit_rows=torch.zeros(0, dtype=torch.long, device=DEV))["logits"]
        assert empty.shape == (0, N_ANS)
        nolab = torch.full_like(feed["input_ids"], -100)
        l_on, l_off = m(**feed, labels=nolab).loss, never(**feed, labels=nolab).loss
        assert torch.isnan(l_on) == torch.isnan(l_off)
        # calls that need every row keep the full decoder: equal to the option-off call
        assert torch.equal(m(**feed)["logits"], ref_full)
        o1, o2 = m(**feed, logit_rows=rows, output_attentions=True), never(**feed, logit_rows=rows, output_attentions=True)
        assert torch.equal(o1["logits"], o2["logits"]) and o1._run.dec_plan is None
        m.engine().eager_logits = never.engine().eager_logits = True
        labels = torch.full_like(feed["input_ids"], -100)
        labels[:, 1] = 7
        e1, e2 = m(**feed, labels=labels), never(**feed, labels=labels)
        assert e1._run.dec_plan is None and torch.equal(e1.loss, e2.loss) and torch.equal(e1.logits, e2.logits)
        m.engine().eager_logits = never.engine().eager_logits = False
        # the option off is bit-identical to a model that never had it
        m.decoder_rows = False
        assert torch.equal(m(**feed, logit_rows=rows)["logits"], ref)


# ------------------------------------------------------------------------------------------------ 4. the loops
def test_videoqa_train_loop_with_decoder_rows(golden):
    from frozenbilm_amd.optim import FusedAdam

    name = "msrvtt"
    g = golden("G10_videoqa", raw=True)
    cfg, P, m = hip_model(N_ANS, 10, g["a2tok"], train=True)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats, decoder_rows=True)
    before = {k: m.get_param(k).detach().clone() for k in DELTA_KEYS}
    opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
    batches = make_videoqa_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, N_ANS, 3, 4, seed=102, dataset_name=name)
    stats = P_vqa.train_one_epoch(m, tok, ListLoader(batches), opt, torch.device(DEV), 0, name, args, max_norm=0.1)
    assert m.decoder_rows is True
    ref = _j(g, f"train_{name}_stats")
    for k in ref:
        assert abs(stats[k] - ref[k]) < 2e-2, (k, stats[k], ref[k])
    for k in DELTA_KEYS:
        d = (m.get_param(k).detach() - before[k]).cpu()
        assert cosine(d, torch.as_tensor(g[f"train_{name}_delta/{k}"])) > 0.9, k


def test_mc_train_loop_with_decoder_rows(golden):
    from frozenbilm_amd.optim import FusedAdam

    g = golden("G11_mc", raw=True)
    cfg, P, m = hip_model(2, 11, g["a2tok"], train=True)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats, decoder_rows=True)
    before = {k: m.get_param(k).detach().clone() for k in DELTA_KEYS}
    opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
    tb = make_mc_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, 4, 3, 4, seed=113)
    stats = P_mc.train_one_epoch(m, tok, ListLoader(tb, mc=4), opt, torch.device(DEV), 0, args, max_norm=0.1)
    assert m.decoder_rows is True
    ref = _j(g, "train_stats")
    for k in ref:
        assert abs(stats[k] - ref[k]) < 2e-2, (k, stats[k], ref[k])
    for k in DELTA_KEYS:
        d = (m.get_param(k).detach() - before[k]).cpu()
        assert cosine(d, torch.as_tensor(g[f"train_delta/{k}"])) > 0.9, k


def test_main_train_and_evaluate_loops_with_decoder_rows(golden):
    """main.train_one_epoch / evaluate with args.decoder_rows against the statistics the reference's own loops recorded (G13)"""
    from frozenbilm_amd import main as P_main
    from frozenbilm_amd.model.config import DebertaV2Config
    from frozenbilm_amd.model.deberta import DebertaV2ForMaskedLM
    from frozenbilm_amd.optim import FusedAdam
    from tests.downstream_fixtures import make_videotext_batches

    g = golden("G13_main_loops", raw=True)
    cfg = _tiny_cfg(max_feats=4, vocab_size=300, max_position_embeddings=128)
    P = O.synth_params(cfg, seed=21, std=0.08, ln_jitter=0.1)
    c = DebertaV2Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        max_position_embeddings=cfg.max_position_embeddings, position_buckets=cfg.position_buckets,
                        layer_norm_eps=cfg.layer_norm_eps, conv_kernel_size=cfg.conv_kernel_size,
                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    m = DebertaV2ForMaskedLM(c, max_feats=cfg.max_feats, features_dim=cfg.features_dim, ds_factor_attn=cfg.ds_factor_attn,
                             ds_factor_ff=cfg.ds_factor_ff, dropout=0.0)
    m.load_state_dict(P, strict=False)
    m.to(DEV)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats, decoder_rows=True)
    batches = make_videotext_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, 3, 6, seed=31)
    torch.manual_seed(7)
    ev = P_main.evaluate(m, tok, ListLoader(batches), torch.device(DEV), args)
    assert m.decoder_rows is True
    ref = _j(g, "eval_stats")
    for k in ref:
        assert abs(ev[k] - ref[k]) < 2e-2, (k, ev[k], ref[k])
    torch.manual_seed(8)
    tr = P_main.train_one_epoch(m, tok, ListLoader(batches), FusedAdam(m, lr=1e-3, betas=(0.9, 0.95)), torch.device(DEV), 0, args, 0.1)
    ref = _j(g, "train_stats")
    for k in ref:
        assert abs(tr[k] - ref[k]) < 2e-2, (k, tr[k], ref[k])


# ------------------------------------------------------------------------------------------------ 5. train mode, dropout live
class _CompactDecoderMasks:
    """tests/dropout_replay.ReplayedMasks, unchanged, behind a wrapper: the row-keyed sites ("hid", "ad") of the last two layer
    executions key by the COMPACT row on the decoder_rows route, so their masks are built at the compact shape and scattered
    into ones at the selected grid rows (what happens on the other rows does not reach the loss).  "pos" and "att" are keyed by
    table row / position and pass through."""

    def __init__(self, inner, grid_rows):
        self.inner, self.grid = inner, grid_rows.cpu()
        self.n = len(inner.execs)

    def _scatter(self, compact, shape):
        full = torch.ones(int(torch.tensor(shape[:-1]).prod()), shape[-1])
        full[self.grid] = compact
        return full.view(*shape)

    def __call__(self, kind, shape):
        from tests.dropout_replay import row_mask

        i, R = self.inner, self.grid.numel()
        if kind == "hid" and i.e_site // 2 >= self.n - 2:
            i.asked.append(kind)
            e, site = i.execs[i.e_site // 2], i.e_site % 2
            i.e_site += 1
            return self._scatter(row_mask(e["hid"][site], (R, shape[-1]), i.p_hid), shape)
        if kind == "ad":
            sites = [s for s in (0, 1) if i.has_ad[s]]
            if i.e_ad // len(sites) >= self.n - 2:
                i.asked.append(kind)
                e, site = i.execs[i.e_ad // len(sites)], sites[i.e_ad % len(sites)]
                i.e_ad += 1
                return self._scatter(row_mask(e["ad"][site], (R, shape[-1]), i.p_ad, ld=e["ldz"][site]), shape)
        return i(kind, shape)

    def exhausted(self):
        return self.inner.exhausted()


def test_train_mode_with_live_dropout_against_the_oracle_with_replayed_masks():
    from tests.dropout_replay import ReplayedMasks

    cfg = _tiny_cfg()
    B, Lt = 4, 40
    P = O.synth_params(cfg, seed=43, std=0.05, ln_jitter=0.1)
    batch = synth_batch(cfg, B=B, L=Lt, seed=9)
    torch.manual_seed(777)
    m = build(cfg, P, train=True)
    m.decoder_rows = True
    out = m(**to_dev(batch))
    run = out._run
    pl = run.dec_plan
    assert pl is not None and run.p_hid > 0 and run.p_att > 0 and run.p_ad > 0 and len(run.layers) == cfg.num_hidden_layers + 1
    c = m.config
    masks = _CompactDecoderMasks(ReplayedMasks(run, cfg, cfg.num_attention_heads, c.hidden_dropout_prob,
                                               c.attention_probs_dropout_prob, m.adapter_dropout), pl.grid)
    gates = []
    n_ex = len(run.layers)
    for e, sv in enumerate(run.layers):
        for z, ds in ((sv.z1, cfg.ds_factor_attn), (sv.z2, cfg.ds_factor_ff)):
            gt = (z[:, : cfg.hidden_size // ds] > 0).cpu()
            if e >= n_ex - 2:  # compact rows -> the grid; the other rows' gates do not reach the loss
                full = torch.ones(B * run.S, gt.shape[1], dtype=torch.bool)
                full[pl.grid.cpu()] = gt
                gt = full
            gates.append(gt)
    out.loss.backward()
    logits = out.logits.float().cpu()
    grads = {n: p.grad.float().cpu().clone() for n, p in m.named_parameters() if p.requires_grad}
    for k, v in P.items():
        v.requires_grad_(O.is_trainable(k))
    with O.bf16_operands(), O.adapter_gates([g_.view(B, -1, g_.shape[-1]) for g_ in gates]), O.dropout_masks(masks):
        ref = O.forward(P, cfg, **batch)
        ref["loss"].backward()
    assert masks.exhausted(), masks.inner.asked
    with torch.no_grad():
        ev = O.forward(P, cfg, **batch)["loss"].item()
    assert abs(ev - ref["loss"].item()) > 1e-3, "dropout made no difference: the comparison would prove nothing"
    sel = pl.grid.cpu()
    dl = abs(out.loss.item() - ref["loss"].item())
    de = (logits.view(B * run.S, -1)[sel] - ref["logits"].reshape(B * run.S, -1)[sel]).abs().max().item()
    worst = sorted(((round((g_ - P[n].grad).norm().item() / max(P[n].grad.norm().item(), 1e-12), 4), n) for n, g_ in grads.items()),
                   reverse=True)
    print(f"[decoder rows, dropout live] loss {out.loss.item():.5f} vs {ref['loss'].item():.5f} (eval-mode oracle {ev:.5f}), "
          f"selected-row logits max-abs {de:.3e}, worst grads {worst[:4]}")
    assert dl < 2e-2 and de < 5e-2 and worst[0][0] < 2e-2, (dl, de, worst[:8])
