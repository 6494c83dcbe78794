"""GPU: fine-tuning through the row-selected prediction head of the DeBERTa engine (``model(..., logit_rows=rows)`` under
autograd) and on packed rows, against the full-logits route, the padded grid, the CPU oracle and the recorded G10 / G11 loops.

Bounds are those of the existing tests of the same comparisons: 2e-3 on logits when only GEMM tile shapes change
(test_inference_graph_replay_matches_the_eager_forward), 1e-4 relative Frobenius on gradients of two routes with the same
arithmetic (test_packed_rows_gradient_through_the_logits), 2e-2 / 3e-2 packed against padded
(test_packed_rows_equal_the_padded_grid_tiny), the oracle bounds of test_gradient_through_logits_vs_oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from frozenbilm_amd import mc as P_mc  # noqa: E402
from frozenbilm_amd import videoqa as P_vqa  # noqa: E402
from frozenbilm_amd.loops import tokenize, video_inputs  # noqa: E402
from oracle import deberta_oracle as O  # noqa: E402
from oracle.model_wrapper import OracleModel  # noqa: E402
from tests.downstream_fixtures import Args, ListLoader, StubTokenizer, make_mc_batches, make_videoqa_batches  # noqa: E402
from tests.golden.make_goldens import _tiny_cfg, synth_batch  # noqa: E402
from tests.test_downstream_loops import DELTA_KEYS, N_ANS, _j, cosine, tiny  # noqa: E402
from tests.test_gpu_downstream import hip_model  # noqa: E402
from tests.test_gpu_model import build, to_dev  # noqa: E402

DEV = "cuda"


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad}


def _worst_rel(got, ref):
    assert got.keys() == ref.keys() and all(r.float().norm().item() > 0 for r in ref.values()), "a reference gradient is zero"
    return max((got[n].float() - ref[n].float()).norm().item() / max(ref[n].float().norm().item(), 1e-12) for n in ref)


def _vqa_feed(cfg, tok, args, B, seed, **kw):
    b = make_videoqa_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, N_ANS, 1, B, seed=seed, **kw)[0]
    video, vmask = video_inputs(b, torch.device(DEV))
    enc = tokenize(tok, b["text"], args)
    feed = dict(video=video, video_mask=vmask, input_ids=enc["input_ids"].to(DEV), attention_mask=enc["attention_mask"].to(DEV))
    return b, enc, feed


def _live_model(cfg, seed, train):
    """the tiny model with its dropout sites live (p = 0.1) and an answer head of cfg.n_ans rows"""
    P = O.synth_params(cfg, seed=seed, std=0.05, ln_jitter=0.1)
    m = build(cfg, P)
    a2tok = torch.randint(1, cfg.vocab_size, (cfg.n_ans, 3), generator=torch.Generator().manual_seed(seed))
    m.set_answer_embeddings(a2tok.to(DEV))
    return m.train(train)


def _forward_at(m, feed, rows, step_seed=0):
    """one forward from a clean gradient state at position `step_seed` of the mask stream; rows None: the full logits"""
    m.zero_grad(set_to_none=True)
    m.step_seed = step_seed
    return m(**feed) if rows is None else m(**feed, logit_rows=rows)


# ------------------------------------------------------------------------------------------------ 1. rows route vs full logits
@pytest.mark.parametrize("train", [False, True])
def test_rows_route_equals_the_full_logits_route(golden, train):
    g = golden("G10_videoqa", raw=True)
    cfg, P, m = hip_model(N_ANS, 10, g["a2tok"], train=train)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats)
    b, enc, feed = _vqa_feed(cfg, tok, args, 6, seed=77)
    rows = P_vqa.mask_rows(enc["input_ids"], tok, args, DEV)
    ans = b["answer_id"].to(DEV)
    full = m(**feed)
    lf = P_vqa.mask_row_logits(full["logits"], enc["input_ids"], tok, args)
    P_vqa.vqa_loss(lf, ans, "msrvtt").backward()
    ref = _grads(m)
    m.zero_grad(set_to_none=True)
    out = m(**feed, logit_rows=rows)
    assert out["loss"] is None and out["logits"].shape == (6, N_ANS) and out["logits"].requires_grad
    assert out._run.pk is None and out._run.N == 6 * (cfg.max_feats + enc["input_ids"].shape[1])
    d_log = (out["logits"].detach() - lf.detach()).abs().max().item()
    P_vqa.vqa_loss(out["logits"], ans, "msrvtt").backward()
    worst = _worst_rel(_grads(m), ref)
    print(f"[rows vs full, train={train}, dropout off] logits max-abs diff {d_log:.3g}, worst gradient Frobenius diff {worst:.3g}")
    assert d_log < 2e-3 and worst < 1e-4


def test_rows_route_equals_the_full_logits_route_with_dropout_live():
    """the head draws no dropout: at the same position of the mask stream both routes draw identical masks"""
    cfg = _tiny_cfg(n_ans=N_ANS)
    m = _live_model(cfg, 71, train=True)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats)
    b, enc, feed = _vqa_feed(cfg, tok, args, 5, seed=78)
    rows = P_vqa.mask_rows(enc["input_ids"], tok, args, DEV)
    ans = b["answer_id"].to(DEV)
    torch.manual_seed(0)
    full = _forward_at(m, feed, None)
    lf = P_vqa.mask_row_logits(full["logits"], enc["input_ids"], tok, args)
    P_vqa.vqa_loss(lf, ans, "msrvtt").backward()
    ref = _grads(m)
    torch.manual_seed(0)
    out = _forward_at(m, feed, rows)
    assert out["logits"].shape == (5, N_ANS) and out["logits"].requires_grad and out._run.p_hid > 0 and out._run.p_ad > 0
    d_log = (out["logits"].detach() - lf.detach()).abs().max().item()
    P_vqa.vqa_loss(out["logits"], ans, "msrvtt").backward()
    worst = _worst_rel(_grads(m), ref)
    m.eval()
    with torch.no_grad():
        d_eval = (m(**feed, logit_rows=rows)["logits"] - lf.detach()).abs().max().item()
    print(f"[rows vs full, dropout live] logits max-abs diff {d_log:.3g}, worst gradient Frobenius diff {worst:.3g} "
          f"(eval-mode logits differ by {d_eval:.3g})")
    assert d_eval > 1e-3  # dropout made a difference
    assert d_log < 2e-3 and worst < 1e-4


# ------------------------------------------------------------------------------------------------ 2. rows + packed vs rows on the grid
def _ragged(cfg, B, Lt, seed):
    """a ragged batch without labels, one requested row inside every sample's valid text, an answer id per sample"""
    batch = synth_batch(cfg, B=B, L=Lt, seed=seed)
    batch.pop("labels")
    S = cfg.max_feats + Lt
    tlen = batch["attention_mask"].sum(1)
    rows = torch.arange(B) * S + cfg.max_feats + tlen // 2
    ans = torch.randint(0, cfg.n_ans, (B,), generator=torch.Generator().manual_seed(seed))
    return to_dev(batch), rows.to(DEV), ans.to(DEV), S


@pytest.mark.parametrize("B,Lt", [(5, 40), (3, 100), (4, 130)])  # S = 50, 110, 140: one, two and three 64-row tiles
def test_packed_rows_route_equals_the_padded_rows_route(B, Lt):
    cfg = _tiny_cfg(n_ans=N_ANS)
    m = _live_model(cfg, 72, train=False)
    feed, rows, ans, S = _ragged(cfg, B, Lt, seed=B + Lt)
    res = {}
    for packed in (False, True):
        m.packed_rows = packed
        m.zero_grad(set_to_none=True)
        out = m(**feed, logit_rows=rows)
        run = out._run
        if packed:
            assert run.pk is not None and run.N == run.pk.n < B * S, "the batch was not packed"
        else:
            assert run.pk is None and run.N == B * S
        assert out["logits"].shape == (B, N_ANS) and out["logits"].requires_grad
        P_vqa.vqa_loss(out["logits"], ans, "msrvtt").backward()
        res[packed] = (out["logits"].detach().clone(), _grads(m), run.N)
    d_log = (res[True][0] - res[False][0]).abs().max().item()
    worst = _worst_rel(res[True][1], res[False][1])
    print(f"[rows packed vs grid S={S}] rows {res[True][2]}/{B * S}, logits max-abs diff {d_log:.3g}, "
          f"worst gradient Frobenius diff {worst:.3g}")
    assert d_log < 2e-2 and worst < 3e-2


def test_packed_rows_route_training_step_is_reproducible_and_finite():
    cfg = _tiny_cfg(n_ans=N_ANS)
    m = _live_model(cfg, 73, train=True)
    m.packed_rows = True
    feed, rows, ans, S = _ragged(cfg, 6, 77, seed=9)
    got = []
    for _ in range(2):
        out = _forward_at(m, feed, rows, step_seed=3)
        assert out._run.pk is not None and out._run.N < 6 * S and out._run.p_hid > 0
        loss = P_vqa.vqa_loss(out["logits"], ans, "msrvtt")
        loss.backward()
        flat = torch.cat([p.grad.reshape(-1) for p in m.parameters() if p.requires_grad]).clone()
        assert torch.isfinite(flat).all() and torch.isfinite(loss) and flat.abs().max().item() > 0
        got.append((out["logits"].detach().clone(), flat))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ------------------------------------------------------------------------------------------------ 3. against the oracle
def test_gradient_through_the_rows_route_packed_vs_oracle(golden):
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
    m.packed_rows = True
    out = m(**feed, logit_rows=P_vqa.mask_rows(enc["input_ids"], tok, args, DEV))
    run = out._run
    assert run.pk is not None and run.N < 6 * run.S and out["loss"] is None and out["logits"].requires_grad
    assert (out["logits"].detach().cpu() - lo.detach()).abs().max().item() < 5e-2
    loss = P_vqa.vqa_loss(out["logits"], b["answer_id"].to(DEV), "msrvtt")
    print(f"[rows packed vs oracle] rows {run.N}/{6 * run.S}, loss {loss.item():.5f} vs {loss_o.item():.5f}")
    assert abs(loss.item() - loss_o.item()) < 2e-2
    loss.backward()
    ref = {n: p.grad for n, p in om.named_ref_parameters().items() if p.requires_grad}
    bad, n, worst = [], 0, 0.0
    for name, p in m.named_parameters():
        if not p.requires_grad:
            continue
        n += 1
        r = ref[name]
        rel = (p.grad.cpu() - r).norm().item() / (r.norm().item() + 1e-12)
        worst = max(worst, rel)
        if rel > (0.25 if "adapter.down" in name else 6e-2):
            bad.append((name, rel))
    print(f"[rows packed vs oracle] worst gradient Frobenius diff {worst:.3g}")
    assert n == len(ref) and not bad, bad[:8]


# ------------------------------------------------------------------------------------------------ 4. mc: C candidates per forward
def test_mc_candidate_scores_on_packed_rows_under_autograd(golden):
    g = golden("G11_mc", raw=True)
    cfg, P, m = hip_model(2, 11, g["a2tok"])
    tok = StubTokenizer(cfg.vocab_size)
    b = make_mc_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, 4, 1, 5, seed=211, min_tok=4, max_tok=40)[0]
    gt = b["answer_id"].to(DEV)
    res = {}
    for key, packed, seq in (("default", False, False), ("packed", True, False), ("packed_seq", True, True)):
        args = Args(max_feats=cfg.max_feats, packed_rows=packed, mc_sequential=seq)
        m.packed_rows = packed
        m.zero_grad(set_to_none=True)
        scores = P_mc.candidate_scores(m, tok, b, torch.device(DEV), args)
        assert scores.shape == (5, 4) and scores.requires_grad
        P_mc.mc_loss(scores, gt, 4).backward()
        res[key] = (scores.detach().clone(), _grads(m))
    for key in ("packed", "packed_seq"):
        d = (res[key][0] - res["default"][0]).abs().max().item()
        worst = _worst_rel(res[key][1], res["default"][1])
        print(f"[mc {key} vs default] scores max-abs diff {d:.3g}, worst gradient Frobenius diff {worst:.3g}")
        assert d < 2e-2 and worst < 3e-2


# ------------------------------------------------------------------------------------------------ 5. the loops
@pytest.mark.parametrize("name", ["msrvtt", "ivqa"])
def test_videoqa_train_loop_on_packed_rows(golden, name):
    from frozenbilm_amd.optim import FusedAdam

    g = golden("G10_videoqa", raw=True)
    cfg, P, m = hip_model(N_ANS, 10, g["a2tok"], train=True)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats, packed_rows=True)
    before = {k: m.get_param(k).detach().clone() for k in DELTA_KEYS}
    opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
    batches = make_videoqa_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, N_ANS, 3, 4, seed=102, dataset_name=name)
    stats = P_vqa.train_one_epoch(m, tok, ListLoader(batches), opt, torch.device(DEV), 0, name, args, max_norm=0.1)
    assert m.packed_rows is True
    ref = _j(g, f"train_{name}_stats")
    for k in ref:
        assert abs(stats[k] - ref[k]) < 2e-2, (k, stats[k], ref[k])
    for k in DELTA_KEYS:
        d = (m.get_param(k).detach() - before[k]).cpu()
        assert cosine(d, torch.as_tensor(g[f"train_{name}_delta/{k}"])) > 0.9, k


def test_mc_train_loop_on_packed_rows(golden):
    from frozenbilm_amd.optim import FusedAdam

    g = golden("G11_mc", raw=True)
    cfg, P, m = hip_model(2, 11, g["a2tok"], train=True)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats, packed_rows=True)
    before = {k: m.get_param(k).detach().clone() for k in DELTA_KEYS}
    opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
    tb = make_mc_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, 4, 3, 4, seed=113)
    stats = P_mc.train_one_epoch(m, tok, ListLoader(tb, mc=4), opt, torch.device(DEV), 0, args, max_norm=0.1)
    assert m.packed_rows is True
    ref = _j(g, "train_stats")
    for k in ref:
        assert abs(stats[k] - ref[k]) < 2e-2, (k, stats[k], ref[k])
    for k in DELTA_KEYS:
        d = (m.get_param(k).detach() - before[k]).cpu()
        assert cosine(d, torch.as_tensor(g[f"train_delta/{k}"])) > 0.9, k


# ------------------------------------------------------------------------------------------------ 6. edges
@pytest.mark.parametrize("packed", [False, True])
def test_rows_route_edges(golden, packed):
    g = golden("G10_videoqa", raw=True)
    cfg, P, m = hip_model(N_ANS, 10, g["a2tok"], train=True)
    m.packed_rows = packed
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats)
    b, enc, feed = _vqa_feed(cfg, tok, args, 4, seed=81)
    b2, enc2, feed2 = _vqa_feed(cfg, tok, args, 3, seed=82)
    rows, rows2 = (P_vqa.mask_rows(e["input_ids"], tok, args, DEV) for e in (enc, enc2))
    ans, ans2 = b["answer_id"].to(DEV), b2["answer_id"].to(DEV)
    n_grid = 4 * (cfg.max_feats + enc["input_ids"].shape[1])

    def one(fd, r, a):
        m.zero_grad(set_to_none=True)
        P_vqa.vqa_loss(m(**fd, logit_rows=r)["logits"], a, "msrvtt").backward()
        return _grads(m)

    # several live runs: two forwards, then one backward each; their gradients add up.  (Every kernel on this path folds in a
    # fixed order, so the only difference to the sum of the two separate steps is the fp32 rounding of one more addition per
    # element, ~1e-7 relative: 1e-5 leaves two orders of magnitude.)
    g1, g2 = one(feed, rows, ans), one(feed2, rows2, ans2)
    m.zero_grad(set_to_none=True)
    o1, o2 = m(**feed, logit_rows=rows), m(**feed2, logit_rows=rows2)
    P_vqa.vqa_loss(o1["logits"], ans, "msrvtt").backward()
    P_vqa.vqa_loss(o2["logits"], ans2, "msrvtt").backward()
    both = _grads(m)
    worst = _worst_rel(both, {n: g1[n] + g2[n] for n in g1})
    print(f"[edges packed={packed}] two live runs vs the sum of two steps: worst gradient Frobenius diff {worst:.3g}")
    assert worst < 1e-5
    # R == 0: [0, n_ans] logits; the backward through them leaves the gradients as they are
    empty = m(**feed, logit_rows=torch.zeros(0, dtype=torch.long, device=DEV))
    assert empty["logits"].shape == (0, N_ANS) and empty["logits"].requires_grad and empty["loss"] is None
    empty["logits"].sum().backward()
    after = _grads(m)
    assert all(torch.equal(after[n], both[n]) for n in both)
    # refused on the host, before the step begins: duplicates, indices outside the grid; labels next to logit_rows
    seed0 = m.step_seed
    for bad in (torch.cat([rows, rows[:1]]), torch.cat([rows[:-1], torch.tensor([n_grid], device=DEV)]),
                torch.tensor([-1], device=DEV)):
        with pytest.raises(ValueError):
            m(**feed, logit_rows=bad)
    labels = torch.full_like(feed["input_ids"], -100)
    labels[:, 1] = 7
    with pytest.raises(RuntimeError):
        m(**feed, logit_rows=rows, labels=labels)
    assert m.step_seed == seed0
    # the no-grad call: untouched -- duplicates allowed, two calls bit-identical, the rows of the full logits
    m.eval()
    m.packed_rows = False
    with torch.no_grad():
        dup = torch.cat([rows, rows[:1]])
        a, b_ = m(**feed, logit_rows=dup)["logits"], m(**feed, logit_rows=dup)["logits"]
        full = P_vqa.mask_row_logits(m(**feed)["logits"], enc["input_ids"], tok, args)
    assert a.shape == (5, N_ANS) and not a.requires_grad and torch.equal(a, b_)
    assert torch.equal(a[:4], full) and torch.equal(a[4], full[0])
