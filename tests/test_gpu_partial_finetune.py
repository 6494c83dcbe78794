"""GPU: partial fine-tuning -- the step, the optimizer and the launch graphs follow `requires_grad`.

Models: the tiny 3-layer model (H = 128, bottleneck 16: the unmerged adapter route) at S = 17 (T = 4, L = 13) and S = 70 (T = 6,
L = 64), and a 2-layer model at the xlarge row width (H = 1536, bottleneck 192: merged route, folded dx, grouped weight-gradient
launches) with B = 2, T = 10, L = 64, as tests/test_gpu_input_grads.py builds them.  Train mode, every dropout site live; the
full step of a (model, shape) is computed once and shared.

Conditions: a pruned step's loss and logits are the full step's bit for bit; so are the gradients of its live leaves (no
exception was needed: every product keeps its launch, its operands and its single writer); a dead parameter has no .grad and
an exactly zero slice of the flat gradient buffer; FusedAdam leaves a dead parameter and its moments alone bit for bit.  Live
parameters after a step: the float64 Adam reference within the per-element bound of tests/test_gpu_rowops.py (imported).  Against
oracle autograd: the project's 2 % relative Frobenius.

Two tests fail without the feature (run on the commit before it): test_freezing_after_the_first_step (the frozen linear_video
still gets its .grad and FusedAdam keeps stepping the flat buffer as a whole) and test_adapter_frozen_before_the_engine_is_built
(seen: KeyError 'deberta.encoder.layer.1.attention.output.adapter.down.weight' -- not in the backward but already while the
engine is built, in _build_trainable_operands: the adapter site looks its parameter up in a table that no longer holds it).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from frozenbilm_amd import train_graph as TG  # noqa: E402
from frozenbilm_amd.optim import FusedAdam  # noqa: E402
from oracle import deberta_oracle as O  # noqa: E402
from tests.gpu_refs import ref_adam  # noqa: E402
from tests.test_gpu_input_grads import BOUND, _batch, _cfg, _dev, _gates_of, _oracle, _params, _rel_fro, build  # noqa: E402
from tests.test_gpu_rowops import C_ADAM, U, judge  # noqa: E402

DEV = "cuda"
SIZES = {"S17": (4, 13, False), "S70": (6, 64, False), "xl": (10, 64, True)}
MID_ADAPTER = "deberta.encoder.layer.1.attention.output.adapter."  # tiny: the middle layer; xl: second parked product of a group
LR, BETAS = 1e-3, (0.9, 0.95)


def cons(m):
    """the trainable-by-construction names (spelled out where the model has no trainable_names(), so that the two tests that
    must fail without the feature fail there for the reason their docstrings give)"""
    if hasattr(m, "trainable_names"):
        return m.trainable_names()
    return [n for n, _ in m.named_parameters() if m._trainable(n)]


def subset(kind, names, nL):
    top = f"deberta.encoder.layer.{nL - 1}."
    return {
        "all": lambda n: True,
        "top_layer": lambda n: n.startswith(top),
        "adapters_only": lambda n: "adapter" in n,
        "layernorms_only": lambda n: "LayerNorm" in n,
        "all_but_linear_video": lambda n: "linear_video" not in n,
        "one_adapter_dead": lambda n: not n.startswith(MID_ADAPTER),
        "conv_layernorm_only": lambda n: n.startswith("deberta.encoder.conv."),  # the conv stage is the lowest that runs
        "top_two": lambda n: n.startswith(top) or n.startswith(f"deberta.encoder.layer.{nL - 2}."),
    }[kind], [n for n in names]


def set_live(m, kind):
    names = cons(m)
    keep, _ = subset(kind, names, m.config.num_hidden_layers)
    named = dict(m.named_parameters())
    live = [n for n in names if keep(n)]
    for n in names:
        named[n].requires_grad_(n in live)
    assert live and (kind == "all" or len(live) < len(names)), kind
    return live


def one_step(m, db, kind, seed=0):
    """one training step from mask-stream position `seed` with the live set `kind`; everything a test compares, cloned"""
    live = set_live(m, kind)
    for p in m.parameters():
        p.grad = None
    m.step_seed = seed
    out = m(**db)
    run = out._run
    saved = len(run.layers)
    out.loss.backward()
    named = dict(m.named_parameters())
    grads = {n: (named[n].grad.detach().clone() if named[n].grad is not None else None) for n in cons(m)}
    eng = m.engine()
    return dict(loss=out.loss.detach().clone(), logits=out.logits.detach().clone(), grads=grads, flat=eng.flat_grad.clone(),
                live=live, saved=saved, run=run)


_MODELS = {}


def model_and_full_step(size):
    """(cfg, model, device batch, host batch, params, the full step, its gates and replayed masks), once per size"""
    if size not in _MODELS:
        from tests.dropout_replay import ReplayedMasks

        T, Lt, xl = SIZES[size]
        cfg = _cfg(T, xl=xl)
        P = _params(cfg, 91)
        batch = _batch(cfg, T, Lt, seed=31, B=2 if xl else 3)
        torch.manual_seed(911)
        m = build(cfg, P, train=True)
        db = _dev(batch)
        set_live(m, "all")
        for p in m.parameters():
            p.grad = None
        m.step_seed = 0
        out = m(**db)
        c = m.config
        masks = ReplayedMasks(out._run, cfg, cfg.num_attention_heads, c.hidden_dropout_prob, c.attention_probs_dropout_prob,
                              m.adapter_dropout)
        gates = _gates_of(out._run, cfg)
        del out
        full = one_step(m, db, "all")
        assert all(g is not None for g in full["grads"].values())
        _MODELS[size] = (cfg, m, db, batch, P, full, gates, masks)
    return _MODELS[size]


# ------------------------------------------------------------------------------------------------ 1. subsets against the full step
@pytest.mark.parametrize("kind", ["top_layer", "adapters_only", "layernorms_only", "all_but_linear_video", "one_adapter_dead",
                                  "conv_layernorm_only"])
@pytest.mark.parametrize("size", list(SIZES))
def test_subset_step_equals_the_full_step(size, kind):
    cfg, m, db, _, _, full, _, _ = model_and_full_step(size)
    eng = m.engine()
    try:
        got = one_step(m, db, kind)
    finally:
        set_live(m, "all")
    assert torch.equal(got["loss"], full["loss"]) and torch.equal(got["logits"], full["logits"])
    live = set(got["live"])
    for n in cons(m):
        o, k = eng.offsets[n], eng.named[n].numel()
        if n in live:
            assert got["grads"][n] is not None and torch.equal(got["grads"][n], full["grads"][n]), f"{kind}: {n} differs from the full step"
        else:
            assert got["grads"][n] is None, f"{kind}: dead {n} has a .grad"
            assert not bool(got["flat"][o:o + k].any()), f"{kind}: flat_grad slice of dead {n} is not zero"
    if kind == "top_layer":  # only the decoder passes were saved
        assert got["saved"] == 2 and full["saved"] == cfg.num_hidden_layers + 1


# ------------------------------------------------------------------------------------------------ 2. the optimizer
def _state(eng, opt):
    return eng.flat.clone(), opt._m.clone(), opt._v.clone()


def _live_mask(eng, live):
    mk = torch.zeros(eng.flat.numel(), dtype=torch.bool, device=DEV)
    for n in live:
        mk[eng.offsets[n]:eng.offsets[n] + eng.named[n].numel()] = True
    return mk


def _ref_step(p64, m64, v64, grad, mk, step, wd=0.0, max_norm=1.0):
    """float64 Adam on the live elements only, clip norm over the live gradient elements"""
    g = torch.where(mk, grad, torch.zeros_like(grad)).double()
    clip = min(1.0, max_norm / (math.sqrt(float((g ** 2).sum())) + 1e-6))
    pl, ml, vl = p64[mk].clone(), m64[mk].clone(), v64[mk].clone()
    ref_adam(pl, g[mk], ml, vl, lr=LR, b1=BETAS[0], b2=BETAS[1], eps=1e-8, wd=wd, step=step, clip=clip)
    p64[mk], m64[mk], v64[mk] = pl, ml, vl


def _fresh(size, seed=92):
    T, Lt, xl = SIZES[size]
    cfg = _cfg(T, xl=xl)
    batch = _batch(cfg, T, Lt, seed=32, B=2 if xl else 3)
    torch.manual_seed(912)
    return cfg, build(cfg, _params(cfg, seed), train=True), _dev(batch)


@pytest.mark.parametrize("kind", ["top_layer", "one_adapter_dead"])
def test_fused_adam_leaves_dead_parameters_alone(kind):
    """step 1 with everything live (so every moment is non-zero), step 2 with the subset: dead p, m, v keep their bits; the live
    ones equal a float64 step on the same gradients with the dead slices zeroed, within fbl_adam_flat's own bound"""
    cfg, m, db = _fresh("S17")
    opt = FusedAdam(m, lr=LR, betas=BETAS, weight_decay=0.01)
    one_step(m, db, "all", seed=0)
    opt.step(clip_max_norm=1.0)
    eng = m.engine()
    p0, m0, v0 = _state(eng, opt)
    assert bool((m0 != 0).any())
    got = one_step(m, db, kind, seed=1)
    mk = _live_mask(eng, got["live"])
    opt.step(clip_max_norm=1.0)
    p1, m1, v1 = _state(eng, opt)
    for a, b, what in ((p0, p1, "p"), (m0, m1, "m"), (v0, v1, "v")):
        assert torch.equal(a[~mk].view(torch.int32), b[~mk].view(torch.int32)), f"dead {what} moved"
    assert bool((p1[mk] != p0[mk]).any())
    p64, m64, v64 = p0.double(), m0.double(), v0.double()
    _ref_step(p64, m64, v64, got["flat"], mk, step=2, wd=0.01)
    judge(f"live parameters after a {kind} step", p1[mk], p64[mk], U * (p0.double().abs()[mk] + LR), C_ADAM)
    norm = math.sqrt(float((got["flat"].double()[mk] ** 2).sum()))
    assert abs(float(opt.grad_norm()) - norm) <= 1e-5 * norm  # the clip norm: over the live elements only


def test_freezing_after_the_first_step():
    """FAILS WITHOUT THE FEATURE: freeze linear_video after one step, run a second one -- its value must not move (it used to keep its .grad
    and FusedAdam stepped the flat buffer as a whole)."""
    cfg, m, db = _fresh("S17")
    opt = FusedAdam(m, lr=LR, betas=BETAS, weight_decay=0.01)
    named = dict(m.named_parameters())
    w, b = named["deberta.embeddings.linear_video.weight"], named["deberta.embeddings.linear_video.bias"]

    def step(seed):
        opt.zero_grad(set_to_none=True)
        m.step_seed = seed
        m(**db).loss.backward()
        opt.step(clip_max_norm=1.0)

    step(0)
    w1, b1 = w.detach().clone(), b.detach().clone()
    w.requires_grad_(False)
    b.requires_grad_(False)
    step(1)
    assert w.grad is None and b.grad is None
    assert torch.equal(w.detach(), w1) and torch.equal(b.detach(), b1), "linear_video moved after it was frozen"
    other = named["deberta.encoder.layer.0.output.LayerNorm.weight"]
    assert other.grad is not None and bool(other.grad.any())


def test_adapter_frozen_before_the_engine_is_built():
    """FAILS WITHOUT THE FEATURE (KeyError while the engine is built): one adapter frozen by hand before the first forward.  Here: it has no
    .grad, it does not move, it keeps its place in the flat layout, and every other gradient is the full model's bit for bit."""
    cfg, m, db, _, _, full, _, _ = model_and_full_step("S17")
    _, m2, _ = _fresh("S17", seed=91)  # (the parameters of the shared model)
    torch.manual_seed(911)
    m2._seed_salt = m._seed_salt
    named = dict(m2.named_parameters())
    dead = [n for n in cons(m2) if n.startswith(MID_ADAPTER)]
    assert len(dead) == 4
    for n in dead:
        named[n].requires_grad_(False)
    assert m2._engine is None
    opt = FusedAdam(m2, lr=LR, betas=BETAS)
    before = {n: named[n].detach().clone() for n in dead}
    m2.step_seed = 0
    out = m2(**_dev(_batch(cfg, *SIZES["S17"][:2], seed=31)))
    out.loss.backward()
    assert torch.equal(out.loss.detach(), full["loss"])
    eng = m2.engine()
    assert eng.offsets == m.engine().offsets and len(opt.param_groups[0]["params"]) == len(cons(m2))
    for n in cons(m2):
        if n in dead:
            assert named[n].grad is None
        else:
            assert torch.equal(named[n].grad, full["grads"][n]), n
    opt.step(clip_max_norm=1.0)
    for n in dead:
        assert torch.equal(named[n].detach(), before[n])
    assert len(opt.state_dict()["state"]) == len(cons(m2)) - 4


def test_refusal_of_a_frozen_lm_weight_at_the_next_forward():
    cfg, m, db, *_ = model_and_full_step("S17")
    name = "deberta.encoder.layer.0.intermediate.dense.weight"
    p = dict(m.named_parameters())[name]
    p.requires_grad_(True)
    try:
        with pytest.raises(NotImplementedError, match="layer.0.intermediate.dense.weight"):
            m(**db)
    finally:
        p.requires_grad_(False)
    with torch.no_grad():
        m(**db)


# ------------------------------------------------------------------------------------------------ 3. against oracle autograd
@pytest.mark.parametrize("kind", ["top_layer", "all_but_linear_video"])
@pytest.mark.parametrize("size", ["S17", "S70"])
def test_subset_gradients_vs_oracle_autograd(size, kind):
    """requires_grad set on the oracle's tensors as on the model's, the masks and gates of the (bit-identical) forward replayed"""
    cfg, m, db, batch, P, full, gates, masks = model_and_full_step(size)
    try:
        got = one_step(m, db, kind)
    finally:
        set_live(m, "all")
    live = set(got["live"])
    for k, v in P.items():
        v.grad = None
        v.requires_grad_(k in live)
    masks.e_pos = masks.e_att = masks.e_site = masks.e_ad = 0
    masks.asked = []
    ref = _oracle(P, cfg, batch, gates, batch["input_ids"].shape[0], masks=masks)
    ref["loss"].backward()
    assert abs(got["loss"].item() - ref["loss"].item()) < 5e-3
    worst = sorted(((round(_rel_fro(got["grads"][n].float().cpu(), P[n].grad), 5), n) for n in live), reverse=True)
    print(f"{size} {kind}: worst live gradients vs oracle {worst[:3]}")
    assert all(P[n].grad is None for n in P if n not in live)
    assert worst[0][0] < BOUND, worst[:8]


# ------------------------------------------------------------------------------------------------ 4. gradual unfreezing
def test_gradual_unfreezing_equals_masked_full_steps():
    """top -> top two -> all.  Per step: the full gradient (all flags on, same seed), then the pruned step and FusedAdam; the
    float64 reference applies Adam with the common step counter to the live elements of the FULL gradient.  state_dict() carries
    states only for parameters that were ever live."""
    cfg, m, db = _fresh("S17")
    opt = FusedAdam(m, lr=LR, betas=BETAS)
    eng = m.engine()
    n_all = len(cons(m))
    p_start = eng.flat.clone()
    p64, m64, v64 = eng.flat.double(), torch.zeros_like(eng.flat).double(), torch.zeros_like(eng.flat).double()
    counts = []
    for t, kind in enumerate(["top_layer", "top_two", "all"], start=1):
        full = one_step(m, db, "all", seed=t)
        got = one_step(m, db, kind, seed=t)
        mk = _live_mask(eng, got["live"])
        assert torch.equal(got["flat"][mk], full["flat"][mk]) and not bool(got["flat"][~mk].any())
        opt.step(clip_max_norm=1.0)
        _ref_step(p64, m64, v64, full["flat"], mk, step=t)
        counts.append(len(opt.state_dict()["state"]))
        if kind != "all":
            assert counts[-1] == len(got["live"]) < n_all
    assert counts[0] < counts[1] < counts[2] == n_all
    judge("parameters after top -> top two -> all", eng.flat, p64, U * (p_start.double().abs() + 3 * LR), C_ADAM)
    sd = opt.state_dict()
    assert all(float(s["step"]) == 3.0 for s in sd["state"].values())
    opt2 = FusedAdam(m, lr=LR, betas=BETAS)
    opt2.load_state_dict(sd)
    assert torch.equal(opt2._m, opt._m) and torch.equal(opt2._v, opt._v) and opt2._step == 3


# ------------------------------------------------------------------------------------------------ 5. memory
def test_a_top_layer_step_holds_less_memory():
    cfg, m, db, *_ = model_and_full_step("S70")
    peak = {}
    try:
        for kind in ("all", "top_layer", "all", "top_layer"):
            set_live(m, kind)
            for p in m.parameters():
                p.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            m.step_seed = 0
            m(**db).loss.backward()
            torch.cuda.synchronize()
            peak[kind] = torch.cuda.max_memory_allocated()
    finally:
        set_live(m, "all")
    print(f"peak memory, tiny model S = 70: full step {peak['all']} bytes, top-layer step {peak['top_layer']} bytes")
    assert peak["top_layer"] < peak["all"]


# ------------------------------------------------------------------------------------------------ 6. launch graphs
@pytest.mark.parametrize("route", ["finetune_graphs", "training_graphs"])
def test_graphs_follow_the_live_set(golden, route):
    """all live -> top layer -> all live, on an eager model and on a graphed one: the change recaptures (a second configuration),
    every step equals the eager step bit for bit, and changing back reuses the first capture."""
    from tests.golden.make_goldens import _tiny_cfg, synth_batch
    from tests.test_downstream_loops import N_ANS
    from tests.test_gpu_model import build as build_m, to_dev

    import torch.nn.functional as F

    ft = route == "finetune_graphs"
    a2tok = golden("G10_videoqa", raw=True)["a2tok"]
    cfg = _tiny_cfg(n_ans=N_ANS if ft else 0)
    B, L = 4, 32  # (the text fills its length bucket: the eager model sees the same batch)
    b = synth_batch(cfg, B=B, L=L, seed=61)
    if ft:
        b.pop("labels")
        rows = (torch.arange(B) * (cfg.max_feats + L) + cfg.max_feats + b["attention_mask"].sum(1) // 2).to(DEV)
        ans = torch.randint(0, N_ANS, (B,), generator=torch.Generator().manual_seed(61)).to(DEV)
    feed = to_dev(b)
    res = []
    for graphs in (False, True):
        torch.manual_seed(321)
        m = build_m(cfg, O.synth_params(cfg, seed=47, std=0.05, ln_jitter=0.1))
        if ft:
            m.set_answer_embeddings(torch.as_tensor(a2tok).to(DEV))
        m.train()
        setattr(m, route, graphs)
        opt = FusedAdam(m, lr=LR, betas=BETAS)
        outs, caps = [], []
        for kind in ("all", "top_layer", "all"):
            set_live(m, kind)
            opt.zero_grad(set_to_none=True)
            if ft:
                lg = m(logit_rows=rows, **feed)["logits"]
                F.cross_entropy(lg, ans).backward()
                outs.append(lg.detach().clone())
            else:
                loss = m(**feed).loss
                loss.backward()
                outs.append(loss.detach().clone())
            opt.step(clip_max_norm=1.0)
            caps.append(TG.stats(m, TG.FINETUNE if ft else TG.MLM).captures)
        res.append((outs, m.engine().flat.clone(), caps, getattr(m, route)))
    (o0, p0, c0, _), (o1, p1, c1, on) = res
    assert c0 == [0, 0, 0] and c1 == [1, 2, 2] and on is True, (c0, c1, on)
    for i in range(3):
        assert torch.equal(o0[i], o1[i]), f"step {i}"
    assert torch.equal(p0, p1)


# ------------------------------------------------------------------------------------------------ 7. BERT
def test_bert_follows_requires_grad():
    from tests import test_gpu_bert as TB

    torch.manual_seed(913)
    m = TB._model(TB._params(TB._ocfg()), train=True)
    db = TB._to(TB._batch())
    names = cons(m)
    named = dict(m.named_parameters())

    def step(seed=0):
        for p in m.parameters():
            p.grad = None
        m.step_seed = seed
        out = m(**db)
        if out.loss.requires_grad:
            out.loss.backward()
        return out

    full_out = step()
    full = {n: named[n].grad.clone() for n in names}
    vid = [n for n in names if "linear_video" in n]
    for n in vid:
        named[n].requires_grad_(False)
    opt = FusedAdam(m, lr=LR, betas=BETAS)
    before = {n: named[n].detach().clone() for n in vid}
    out = step()
    assert torch.equal(out.loss.detach(), full_out.loss.detach())
    for n in names:
        if n in vid:
            assert named[n].grad is None
        else:
            assert torch.equal(named[n].grad, full[n]), n
    # the top layer only: the backward stops below it, the rest is neither saved nor touched
    top = f"bert.encoder.layer.{m.config.num_hidden_layers - 1}."
    for n in names:
        named[n].requires_grad_(n.startswith(top))
    out = step()
    for n in names:
        assert (named[n].grad is None) != n.startswith(top)
        if n.startswith(top):
            assert torch.equal(named[n].grad, full[n]), n
    # FusedAdam leaves the frozen linear_video where it is
    for n in names:
        named[n].requires_grad_(n not in vid)
    step()
    opt.step(clip_max_norm=1.0)
    for n in vid:
        assert torch.equal(named[n].detach(), before[n])
    # nothing live: a grad-mode call in train mode runs, and returns no grad function
    for n in names:
        named[n].requires_grad_(False)
    with torch.no_grad():
        m.step_seed = 0
        full_out = m(**db)
    out = step()
    assert out.loss.grad_fn is None and not out.loss.requires_grad
    assert torch.equal(out.loss.detach(), full_out.loss.detach())
