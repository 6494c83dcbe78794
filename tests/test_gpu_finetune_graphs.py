"""GPU: the fine-tuning step as two replayed launch graphs (``model.finetune_graphs``, train_graph.FinetuneStep).

A replayed step runs the kernels of the eager step on the batch padded to its length bucket, with the same seeds: every
comparison against "the eager step" below feeds the eager model the test's own padded copy of the batch and the remapped
rows, and asks for bit-for-bit equality (torch.equal) -- of the logits after every step, of every trainable parameter after
the optimizer steps.  Tiny dimensions throughout (tests/golden/make_goldens._tiny_cfg, the G10 / G11 answer tables)."""
import os
import socket
import subprocess
import sys
import types
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from frozenbilm_amd import mc as P_mc  # noqa: E402
from frozenbilm_amd import train_graph as TG  # noqa: E402
from frozenbilm_amd import videoqa as P_vqa  # noqa: E402
from frozenbilm_amd.optim import FusedAdam  # noqa: E402
from oracle import deberta_oracle as O  # noqa: E402
from tests.downstream_fixtures import Args, ListLoader, StubTokenizer, make_mc_batches, make_videoqa_batches  # noqa: E402
from tests.golden.make_goldens import _tiny_cfg, synth_batch  # noqa: E402
from tests.test_downstream_loops import DELTA_KEYS, N_ANS, _j, cosine  # noqa: E402
from tests.test_gpu_downstream import hip_model  # noqa: E402
from tests.test_gpu_model import _rel_fro, build, to_dev  # noqa: E402

DEV = "cuda"
BUCKET = 32


def _live_model(a2tok, seed=47, torch_seed=321):
    """the tiny model (T = 10) with every dropout site live, the G10 answer table as its head, in training mode"""
    cfg = _tiny_cfg(n_ans=N_ANS)
    torch.manual_seed(torch_seed)  # (salts the model's mask stream at its first training forward)
    m = build(cfg, O.synth_params(cfg, seed=seed, std=0.05, ln_jitter=0.1))
    m.set_answer_embeddings(torch.as_tensor(a2tok).to(DEV))
    return cfg, m.train()


def _batch(cfg, B, L, seed):
    """ragged batch without labels, one requested row inside every sample's valid text, an answer per sample"""
    b = synth_batch(cfg, B=B, L=L, seed=seed)
    b.pop("labels")
    tlen = b["attention_mask"].sum(1)
    rows = torch.arange(B) * (cfg.max_feats + L) + cfg.max_feats + tlen // 2
    ans = torch.randint(0, N_ANS, (B,), generator=torch.Generator().manual_seed(seed))
    return to_dev(b), rows.to(DEV), ans.to(DEV)


def _padded(cfg, feed, rows):
    """the test's own copy of the batch on its length bucket: pad tokens with mask 0 behind the text, rows moved along"""
    L = feed["input_ids"].shape[1]
    Lp = -(-L // BUCKET) * BUCKET
    out = dict(feed, input_ids=F.pad(feed["input_ids"], (0, Lp - L), value=0), attention_mask=F.pad(feed["attention_mask"], (0, Lp - L), value=0))
    S, Sp = cfg.max_feats + L, cfg.max_feats + Lp
    return out, (rows // S) * Sp + rows % S


def _zero(m, opt, set_to_none):
    if set_to_none:
        for p in m.parameters():
            p.grad = None
    else:
        opt.zero_grad(set_to_none=False)


def _params(m):
    return {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad}


def _step(m, opt, feed, rows, ans, set_to_none=False):
    _zero(m, opt, set_to_none)
    logits = m(logit_rows=rows, **feed)["logits"]
    F.cross_entropy(logits, ans).backward()
    opt.step(clip_max_norm=1.0)
    return logits.detach().clone()


def _replays(m):
    return TG.stats(m, TG.FINETUNE).replays


def _cache(m):
    return m.__dict__.get("_finetune_graph_cache", {})


# ------------------------------------------------------------------------------------------------ 1. replay == eager step
@pytest.mark.parametrize("set_to_none", [True, False])
def test_replayed_finetune_step_equals_the_eager_step(golden, set_to_none):
    """B = 4 at L = 21 and L = 32 share the bucket of 32 (one capture), B = 3 at L = 40 lands in the bucket of 64 (a second
    capture, made while the flat gradient buffer holds the gradients of step 2)."""
    a2tok = golden("G10_videoqa", raw=True)["a2tok"]
    results = []
    for graphs in (False, True):
        cfg, m = _live_model(a2tok)
        m.finetune_graphs = graphs
        opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
        logits = []
        for i, (B, L) in enumerate([(4, 21), (4, 32), (3, 40)]):
            feed, rows, ans = _batch(cfg, B, L, seed=60 + i)
            if not graphs:
                feed, rows = _padded(cfg, feed, rows)
            logits.append(_step(m, opt, feed, rows, ans, set_to_none))
            assert logits[-1].shape == (B, N_ANS)
        results.append((logits, _params(m), m.step_seed))
        if graphs:  # the two assertions that cannot hold without the feature
            assert len(_cache(m)) == 2 and TG.stats(m, TG.FINETUNE).captures == 2, list(_cache(m))
            assert _replays(m) == 3
            assert m.finetune_graphs is True
        else:
            assert not _cache(m) and _replays(m) == 0
    (l0, p0, s0), (l1, p1, s1) = results
    assert s0 == s1 == 3
    for i in range(3):
        assert torch.equal(l0[i], l1[i]), f"logits of step {i}: max-abs diff {(l0[i] - l1[i]).abs().max().item():.3g}"
    assert not torch.equal(l0[0][:3], l0[2])  # (three different steps)
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n


# ------------------------------------------------------------------------------------------------ 2. edges
def test_finetune_graph_edges(golden):
    a2tok = golden("G10_videoqa", raw=True)["a2tok"]
    cfg, m = _live_model(a2tok)
    _, twin = _live_model(a2tok)  # the eager run: padded copies, never served by a graph
    m.finetune_graphs = True
    opt, opt_t = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95)), FusedAdam(twin, lr=1e-3, betas=(0.9, 0.95))
    feed, rows, ans = _batch(cfg, 4, 21, seed=81)
    pfeed, prows = _padded(cfg, feed, rows)

    def both_steps():
        a, b = _step(m, opt, feed, rows, ans), _step(twin, opt_t, pfeed, prows, ans)
        assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(_params(m).values(), _params(twin).values()))

    both_steps()
    assert _replays(m) == 1
    # a second graphed forward while the first output's backward is pending is refused: the graph owns one set of activations
    opt.zero_grad(set_to_none=False)
    out = m(logit_rows=rows, **feed)["logits"]
    with pytest.raises(RuntimeError, match="before backward"):
        m(logit_rows=rows, **feed)
    assert _replays(m) == 2 and m.step_seed == 2
    # a None gradient replays nothing and leaves the backward pending
    step = next(iter(_cache(m).values()))
    g0 = m.engine().flat_grad.clone()
    got = TG._Replay.backward(types.SimpleNamespace(step=step), None)
    assert all(x is None for x in got) and step.pending_backward and torch.equal(g0, m.engine().flat_grad)
    F.cross_entropy(out, ans).backward()
    opt.step(clip_max_norm=1.0)
    opt_t.zero_grad(set_to_none=False)
    F.cross_entropy(twin(logit_rows=prows, **pfeed)["logits"], ans).backward()
    opt_t.step(clip_max_norm=1.0)
    # an eval no_grad forward and an inference-graph forward in between do not disturb the captured step
    m.eval()
    with torch.no_grad():
        ev = m(logit_rows=rows, **feed)["logits"]
        m.inference_graphs = True
        ev_g = m(logit_rows=rows, **feed)["logits"]
        m.inference_graphs = False
    assert m.__dict__.get("_graph_cache") and (ev - ev_g).abs().max().item() < 2e-3 and m.step_seed == 2
    m.train()
    both_steps()
    # the output dropped without backward: the next forward is refused until the caller says so (drop_pending_backward)
    opt.zero_grad(set_to_none=False)
    m(logit_rows=rows, **feed)
    twin(logit_rows=prows, **pfeed)  # (the eager run draws -- and drops -- the same step of its mask stream)
    with pytest.raises(RuntimeError):
        m(logit_rows=rows, **feed)
    TG.drop_pending_backward(m)
    both_steps()
    # duplicate rows are refused on the host before anything is replayed
    n_rep, seed0 = _replays(m), m.step_seed
    with pytest.raises(ValueError, match="more than once"):
        m(logit_rows=torch.cat([rows, rows[:1]]), **feed)
    with pytest.raises(ValueError, match="token grid"):
        m(logit_rows=torch.cat([rows[:-1], torch.tensor([4 * (cfg.max_feats + 21)], device=DEV)]), **feed)
    assert _replays(m) == n_rep and m.step_seed == seed0 and not step.pending_backward
    # packed rows take the eager path
    m.packed_rows = True
    opt.zero_grad(set_to_none=False)
    out = m(logit_rows=rows, **feed)
    assert _replays(m) == n_rep and out["logits"].requires_grad and out._run.pk is not None
    F.cross_entropy(out["logits"], ans).backward()
    m.packed_rows = False
    assert len(_cache(m)) == 1
    # a rebuilt engine drops the captured steps; the next step captures again and is served
    m.set_answer_embeddings(torch.as_tensor(a2tok).to(DEV))
    assert "_finetune_graph_cache" not in m.__dict__
    m.train()
    opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
    _step(m, opt, feed, rows, ans)
    assert _replays(m) == n_rep + 1 and len(_cache(m)) == 1 and TG.stats(m, TG.FINETUNE).captures == 1


# ------------------------------------------------------------------------------------------------ 3. mc.candidate_scores
class _BucketTokenizer(StubTokenizer):
    """pads every tokenized batch to its length bucket: `mc.candidate_scores` then builds the padded batch itself"""

    def __call__(self, text, **kw):
        enc = super().__call__(text, **kw)
        L = enc["input_ids"].shape[1]
        return {k: F.pad(v, (0, -(-L // BUCKET) * BUCKET - L), value=0) for k, v in enc.items()}


def test_mc_candidate_scores_through_the_graphs(golden):
    """three candidates of B = 2 questions in one forward of six samples (R = 6)"""
    g = golden("G11_mc", raw=True)
    cfg, P, m = hip_model(2, 11, g["a2tok"], train=True)
    b = make_mc_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, 3, 1, 2, seed=211, min_tok=4, max_tok=20)[0]
    gt = b["answer_id"].to(DEV)
    res = {}
    for graphs in (False, True):
        m.finetune_graphs = graphs
        tok = StubTokenizer(cfg.vocab_size) if graphs else _BucketTokenizer(cfg.vocab_size)
        m.zero_grad(set_to_none=True)
        scores = P_mc.candidate_scores(m, tok, b, torch.device(DEV), Args(max_feats=cfg.max_feats, train_logit_rows=True))
        assert scores.shape == (2, 3) and scores.requires_grad
        P_mc.mc_loss(scores, gt, 3).backward()
        res[graphs] = (scores.detach().clone(), _grads(m))
    assert _replays(m) == 1 and next(iter(_cache(m).values())).static["rows"].numel() == 6
    assert torch.equal(res[True][0], res[False][0])
    for n, ref in res[False][1].items():
        assert ref.abs().max().item() > 0 and torch.equal(res[True][1][n], ref), n


# ------------------------------------------------------------------------------------------------ 4. the loops
@pytest.mark.parametrize("name", ["msrvtt", "ivqa"])
def test_videoqa_train_loop_on_finetune_graphs(golden, name):
    """the recorded statistics and the bound of test_videoqa_train_loop_on_packed_rows"""
    g = golden("G10_videoqa", raw=True)
    cfg, P, m = hip_model(N_ANS, 10, g["a2tok"], train=True)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats, finetune_graphs=True)
    before = {k: m.get_param(k).detach().clone() for k in DELTA_KEYS}
    opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
    batches = make_videoqa_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, N_ANS, 3, 4, seed=102, dataset_name=name)
    stats = P_vqa.train_one_epoch(m, tok, ListLoader(batches), opt, torch.device(DEV), 0, name, args, max_norm=0.1)
    assert m.finetune_graphs is True and _replays(m) == 3 and len(_cache(m)) == 1
    ref = _j(g, f"train_{name}_stats")
    for k in ref:
        print(f"[videoqa {name} loop on graphs] {k}: {stats[k]:.5f} (recorded {ref[k]:.5f})")
        assert abs(stats[k] - ref[k]) < 2e-2, (k, stats[k], ref[k])
    for k in DELTA_KEYS:
        d = (m.get_param(k).detach() - before[k]).cpu()
        assert cosine(d, torch.as_tensor(g[f"train_{name}_delta/{k}"])) > 0.9, k


def test_mc_train_loop_on_finetune_graphs(golden):
    """the recorded statistics and the bound of test_mc_train_loop_on_packed_rows"""
    g = golden("G11_mc", raw=True)
    cfg, P, m = hip_model(2, 11, g["a2tok"], train=True)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=cfg.max_feats, finetune_graphs=True)
    before = {k: m.get_param(k).detach().clone() for k in DELTA_KEYS}
    opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
    tb = make_mc_batches(cfg.vocab_size, cfg.max_feats, cfg.features_dim, 4, 3, 4, seed=113)
    stats = P_mc.train_one_epoch(m, tok, ListLoader(tb, mc=4), opt, torch.device(DEV), 0, args, max_norm=0.1)
    assert m.finetune_graphs is True and _replays(m) == 3
    ref = _j(g, "train_stats")
    for k in ref:
        print(f"[mc loop on graphs] {k}: {stats[k]:.5f} (recorded {ref[k]:.5f})")
        assert abs(stats[k] - ref[k]) < 2e-2, (k, stats[k], ref[k])
    for k in DELTA_KEYS:
        d = (m.get_param(k).detach() - before[k]).cpu()
        assert cosine(d, torch.as_tensor(g[f"train_delta/{k}"])) > 0.9, k


# ------------------------------------------------------------------------------------------------ 5. shape churn
def test_shape_churn_switches_the_graphs_off_with_one_warning(golden):
    """MAX_CAPTURES = 12 distinct configurations are captured; the thirteenth (here: batch sizes 1 .. 13, and a second length
    bucket among them) switches the feature off with one warning and training goes on eagerly"""
    assert TG.MAX_CAPTURES == 12
    a2tok = golden("G10_videoqa", raw=True)["a2tok"]
    cfg, m = _live_model(a2tok)
    m.finetune_graphs = True
    opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for B in range(1, 16):
            _step(m, opt, *_batch(cfg, B, 40 if B == 5 else 9, seed=B))
            assert torch.isfinite(m.engine().flat_grad).all() and m.engine().flat_grad.abs().max().item() > 0
            assert m.finetune_graphs is (B <= 12), B
    said = [w for w in seen if "finetune_graphs" in str(w.message)]
    assert len(said) == 1 and "13 distinct" in str(said[0].message), [str(w.message) for w in seen]
    assert _replays(m) == 12 and not _cache(m) and TG.stats(m, TG.FINETUNE).auto_off is True
    assert m.step_seed == 15


# ------------------------------------------------------------------------------------------------ 6. consistency over replays
def test_finetune_graphs_100_replays(golden):
    """One shape, 100 optimizer steps served by one pair of graphs: the flat gradient buffer is finite after every backward
    replay (counted on the device, read back once at the end) and steps 1, 50 and 100 equal the eager step from the same
    state bit for bit (modelled on test_graphed_training_step_soak_300_replays, at the tiny dimensions)."""
    a2tok = golden("G10_videoqa", raw=True)["a2tok"]
    cfg, m = _live_model(a2tok)
    opt = FusedAdam(m, lr=3e-4, betas=(0.9, 0.95))
    feed, rows, ans = _batch(cfg, 4, 21, seed=5)
    pfeed, prows = _padded(cfg, feed, rows)
    m.finetune_graphs = True
    n = 100
    nf = torch.zeros(n, dtype=torch.int32, device=DEV)
    mism = []
    for i in range(n):
        seed_before = m.step_seed
        opt.zero_grad(set_to_none=False)
        logits = m(logit_rows=rows, **feed)["logits"]
        F.cross_entropy(logits, ans).backward()
        g = m.engine().flat_grad
        nf[i] = (~torch.isfinite(g)).sum() + (~torch.isfinite(logits.detach())).sum()
        if i + 1 in (1, 50, 100):
            g_rep, l_rep = g.clone(), logits.detach().clone()
            m.finetune_graphs = False
            m.step_seed = seed_before
            opt.zero_grad(set_to_none=False)
            l2 = m(logit_rows=prows, **pfeed)["logits"]
            F.cross_entropy(l2, ans).backward()
            if not (torch.equal(g_rep, m.engine().flat_grad) and torch.equal(l_rep, l2.detach())):
                mism.append(i + 1)
            m.finetune_graphs = True
            g.copy_(g_rep)
        opt.step(clip_max_norm=0.1)
    bad = nf.cpu()
    assert int(bad.sum()) == 0, f"non-finite gradient in replay {int(torch.nonzero(bad)[0])}"
    assert not mism, mism
    assert TG.stats(m, TG.FINETUNE).captures == 1 and _replays(m) == n


# ------------------------------------------------------------------------------------------------ 7. a released cache
@pytest.mark.parametrize("route", TG.ROUTES, ids=lambda r: r.switch)
def test_a_cache_popped_by_its_name_is_captured_again(golden, route):
    """All three routes at B = 2, 10 video slots, 21 text tokens: two served calls, the route's cache popped from
    `model.__dict__` by its name (what the benchmark does to release the graphs), the same feed again.  The third call
    captures anew and is served; it returns what the second returned (inference: same weights, same feed) or what an eager
    twin stepped alongside returns (training routes: loss / logits and the flat gradient buffer), bit for bit."""
    a2tok = golden("G10_videoqa", raw=True)["a2tok"]
    cfg, m = _live_model(a2tok)
    setattr(m, route.switch, True)
    st = TG.stats(m, route)
    labelled = to_dev(synth_batch(cfg, B=2, L=21, seed=91))
    feed, rows, ans = _batch(cfg, 2, 21, seed=91)
    pfeed, prows = _padded(cfg, feed, rows)

    def call(model, graphed):
        """one call of the route's kind: its output, and the flat gradient it left"""
        if route is TG.INFERENCE:
            with torch.no_grad():
                return model(logit_rows=rows, **feed)["logits"].clone(), None
        model.zero_grad(set_to_none=False)
        if route is TG.MLM:
            out = model(mlm=True, **labelled).loss
            out.backward()
        else:
            out = model(logit_rows=rows, **feed)["logits"] if graphed else model(logit_rows=prows, **pfeed)["logits"]
            F.cross_entropy(out, ans).backward()
        return out.detach().clone(), model.engine().flat_grad.clone()

    if route is TG.INFERENCE:
        m.eval()
        twin = None
    else:
        _, twin = _live_model(a2tok)  # the eager run (the fine-tuning route: on the padded copy of the batch)
    outs = []
    for i in range(3):
        if i == 2:
            assert st.replays == 2 and len(m.__dict__.pop(route.cache)) == 1
        outs.append(call(m, True))
        if twin is not None:
            ref = call(twin, False)
            assert torch.equal(outs[-1][0], ref[0]) and torch.equal(outs[-1][1], ref[1]), i
            assert ref[1].abs().max().item() > 0
    assert len(m.__dict__[route.cache]) == 1 and st.replays == 3 and getattr(m, route.switch) is True
    assert st.captures == (1 if route.budgeted else 0)  # (captured twice; a configuration seen before is not counted again)
    if route is TG.INFERENCE:
        assert torch.equal(outs[2][0], outs[1][0]) and outs[2][0].shape == (2, N_ANS)
    else:
        assert not torch.equal(outs[2][0], outs[1][0])  # (another step of the mask stream)


# ------------------------------------------------------------------------------------------------ 8. two ranks
CHILD_LIMIT_S = 240


def _run_two_ranks(tmp_path):
    """both ranks on one GPU over gloo; each child has its own time limit, and when one exceeds it both are killed and
    nothing further is started"""
    world = 2
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    out_file = str(tmp_path / "finetune_graphs_dp.pt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "finetune_graphs_dp_worker.py"), out_file],
                                      env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs, timed_out = [], False
    for p_ in procs:
        try:
            o, _ = p_.communicate(timeout=1 if timed_out else CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            timed_out = True
            for q in procs:
                q.kill()
            o, _ = p_.communicate()
        logs.append(o)
    assert not timed_out, "a rank exceeded its time limit; both were killed\n" + "\n".join(logs)
    assert all(p_.returncode == 0 for p_ in procs), "\n".join(logs)
    print("\n".join(l for lg in logs for l in lg.splitlines() if "[finetune_graphs_dp_worker]" in l))
    return torch.load(out_file)


def test_two_rank_finetune_graph_replay_beside_an_eager_rank(tmp_path):
    """model.finetune_graphs on both ranks; rank 1's capture budget is used up, so it serves every step eagerly while rank 0
    replays: both issue one all-reduce over the whole flat buffer per step ("after" placement), and the reduced gradients equal
    the single-process gradients of the concatenated batch (mean over ranks of the per-rank mean loss) to the 1e-5 relative
    Frobenius bound of test_two_rank_data_parallel_equivalence_on_the_hip_engine.  The text is one full bucket long (L = 32):
    a rank that fell back runs its shard unpadded, so only there do both ranks -- and the single process -- work on one grid
    and the fp32-rounding bound applies; padding itself is covered by test_replayed_finetune_step_equals_the_eager_step."""
    from tests.finetune_graphs_dp_worker import make_inputs, make_model

    got = _run_two_ranks(tmp_path)
    assert got["ranks_agree"] and got["world"] == 2 and got["pattern_same"], got
    assert got["collectives"] == 1 and got["overlap"] == "after" and got["served"] == ["graph", "eager"], got
    assert got["replays"] == [2, 0]
    cfg, m = make_model()
    m.zero_grad(set_to_none=False)
    for r in range(2):
        feed, rows, ans = make_inputs(cfg, r, 2, DEV)
        F.cross_entropy(m(logit_rows=rows, **feed)["logits"], ans).backward()
    want = {n: p.grad.float().cpu() / 2 for n, p in m.named_parameters() if p.requires_grad}
    worst = max(_rel_fro(got["grads"][n], want[n]) for n in want)
    print(f"worst relative difference reduced (graph + eager rank) vs single-process: {worst:.2e}")
    assert worst < 1e-5, worst
