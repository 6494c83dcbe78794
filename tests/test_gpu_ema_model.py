"""GPU: the moving average of the trainable weights at model level -- FusedAdam(..., ema_decay=), model.ema_weights(), the loops
and the checkpoints -- on the tiny 3-layer DeBERTa at S = 17 and the tiny BERT, as tests/test_gpu_optim_groups.py builds them
(its `Model` is imported): four training steps from fixed seeds, every dropout site live, the clip on.

Bit equalities are conditions.  The one bound is that of the average against the float64 recurrence over the recorded post-step
parameters: the per-update bound of tests/ema_cases.py, 2^-24 (w |p - e| + |ref|) (1 + 2^-20), accumulated over the four updates
as B_k = (1 - w_k) B_{k-1} + bound(e_{k-1}, p_k, w_k), B_0 = 0 (ema_cases.accumulated_bound: one update maps the kernel's average
and the reference by the same affine map up to the kernel's two roundings) -- no element outside.

 1. trajectory: with ema_decay = 0.9 the loss of every step and p, m, v after the last are those of the run without EMA, for
    the plain optimizer, for two parameter groups with AdamW decay, and for a run that freezes one layer's adapters after step 2
    (there the frozen slice of the average keeps the bits it had at step 2);
 2. the average against the recurrence (with and without warm-up);
 3. inside `with model.ema_weights():` in eval mode the logits are those of a fresh model loaded with ema_state_dict(), and not
    those outside it; the same through a captured inference graph;
 4. leaving restores every bit, and the next training step is that of a run that never entered;
 5. step(), a nested entry, merge_lora() (LoRA model), optimizer.state_dict() / load_state_dict() and model.load_state_dict()
    inside the context raise RuntimeError;
 6. checkpoint round trip through save_checkpoint, into FusedAdam with and without EMA and into torch.optim.Adam; with
    ema_weights=True the file's "model" entry is the averaged model;
 7. main.evaluate with args.eval_ema gives the loss of the fresh averaged model and leaves the training parameters alone;
 8. BERT: conditions 1 (plain), 3 and 4.

On the parent commit every test fails at its first FusedAdam(..., ema_decay=): TypeError, __init__() got an unexpected keyword
argument 'ema_decay' (seen there)."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from frozenbilm_amd.optim import FusedAdam  # noqa: E402
from tests import ema_cases as EC  # noqa: E402
from tests.test_gpu_optim_groups import Model, bits  # noqa: E402

DEV = "cuda"
LR, BETAS, WD, DECAY, MAX_NORM, STEPS = 1e-3, (0.9, 0.95), 0.01, 0.9, 1.0, 4
FROZEN = "deberta.encoder.layer.1."  # the freezing run: this layer's adapters stop training after step 2


def optimizer(M, kind, **ema):
    if kind == "groups":  # two groups, AdamW decay: LayerNorms at half the rate without decay
        return FusedAdam(M.m, lr=LR, betas=BETAS, weight_decay=WD, decoupled_weight_decay=True,
                         param_groups=[dict(params=[]), dict(params=["*LayerNorm*"], lr=0.5 * LR, weight_decay=0.0)], **ema)
    return FusedAdam(M.m, lr=LR, betas=BETAS, weight_decay=WD, **ema)


def train(M, opt, first=0, steps=STEPS, freeze_after=None):
    """training steps first .. first + steps - 1 (the step number is the position in the mask stream); what a test compares:
    the losses, and the flat buffer and the average after every step"""
    M.m.train()
    losses, flats, emas = [], [], []
    for k in range(first, first + steps):
        for p in M.m.parameters():
            p.grad = None
        M.m.step_seed = k
        out = M.m(**M.db)
        out.loss.backward()
        opt.step(clip_max_norm=MAX_NORM)
        losses.append(out.loss.detach().clone())
        flats.append(M.m.engine().flat.clone())
        emas.append(opt._ema.clone() if opt._ema is not None else None)
        if freeze_after == k + 1:
            for n in M.names:
                if n.startswith(FROZEN) and "adapter" in n:
                    M.named[n].requires_grad_(False)
    torch.cuda.synchronize()
    return losses, flats, emas


def run(size, kind="plain", freeze_after=None, **ema):
    M = Model(size)
    start = M.m.engine().flat.clone()
    opt = optimizer(M, kind, **ema)
    return (M, opt, start, *train(M, opt, freeze_after=freeze_after))


def same_trajectory(a, b):
    (Ma, oa, _, la, fa, _), (Mb, ob, _, lb, fb, _) = a, b
    for k, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), f"the loss of step {k + 1} differs: {x.item()!r} against {y.item()!r}"
    assert torch.equal(bits(fa[-1]), bits(fb[-1])), "the parameters differ"
    assert torch.equal(bits(oa._m), bits(ob._m)) and torch.equal(bits(oa._v), bits(ob._v)), "the moments differ"
    assert oa._step == ob._step == len(la)


_RUNS = {}


def ema_run(size):
    """the plain EMA run of a model (four steps), shared by the tests that only read it"""
    if size not in _RUNS:
        _RUNS[size] = run(size, ema_decay=DECAY)
    return _RUNS[size]


def fresh_averaged(size, opt):
    """a fresh model loaded with the exported average, in eval mode"""
    F = Model(size)
    sd = opt.ema_state_dict()
    assert list(sd) == F.m.trainable_names() and all(v.dtype is torch.float32 and v.shape == F.named[n].shape for n, v in sd.items())
    missing, unexpected = F.m.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing).isdisjoint(sd)
    return F.m.eval()


def feeds(M):
    feed = {k: v for k, v in M.db.items() if k != "labels"}
    S = feed["video"].shape[1] + feed["input_ids"].shape[1]
    rows = torch.tensor([1 + feed["video"].shape[1], S + 2 + feed["video"].shape[1]], device=DEV)  # a text row of samples 0 and 1
    return feed, rows


# ------------------------------------------------------------------------------------------------ 1. trajectory
@pytest.mark.parametrize("kind", ["plain", "groups", "freeze"])
def test_trajectory_is_that_of_the_run_without_ema(kind):
    kw = dict(kind="plain", freeze_after=2) if kind == "freeze" else dict(kind=kind)
    with_ema = run("S17", **kw, ema_decay=DECAY)
    same_trajectory(with_ema, run("S17", **kw))
    M, opt, start, _, flats, emas = with_ema
    assert opt.ema_updates == STEPS and opt.has_ema
    eng = M.m.engine()
    frozen = torch.zeros_like(start, dtype=torch.bool)
    for n in M.names:
        if kind == "freeze" and n.startswith(FROZEN) and "adapter" in n:
            frozen[slice(*M.span(n))] = True
    assert bool(frozen.any()) == (kind == "freeze")
    # the frozen layer's slice: the bits of step 2, in the average as in the parameters; everything else went on moving
    assert torch.equal(bits(emas[3])[frozen], bits(emas[1])[frozen]) and torch.equal(bits(flats[3])[frozen], bits(flats[1])[frozen])
    if kind == "freeze":
        assert not torch.equal(bits(emas[1])[frozen], bits(start)[frozen]), "the frozen adapters never trained"
        assert not eng.all_live
    for n in M.names:  # (the other layers' adapters, name by name)
        b, e = M.span(n)
        if "adapter" in n and n.endswith(".weight") and not bool(frozen[b]):
            assert not torch.equal(bits(emas[3][b:e]), bits(emas[1][b:e])), f"the average of {n} stopped moving"
    assert not torch.equal(bits(emas[3])[~frozen], bits(emas[1])[~frozen])


# ------------------------------------------------------------------------------------------------ 2. the average
@pytest.mark.parametrize("warmup", [False, True], ids=["constant", "warmup"])
def test_average_against_the_float64_recurrence(warmup):
    M, opt, start, _, flats, emas = ema_run("S17") if not warmup else run("S17", ema_decay=DECAY, ema_warmup=True)
    ws = [EC.weight(DECAY, u, warmup) for u in range(1, STEPS + 1)]
    assert ws == ([1 - DECAY] * 4 if not warmup else [1 - 2 / 11, 1 - 3 / 12, 1 - 4 / 13, 1 - 5 / 14])
    before = [start] + emas[:-1]  # the kernel's average in front of every update; the first one is the initial parameters
    ref = EC.recurrence(start, flats, ws)
    B = EC.accumulated_bound(before, flats, ws)
    err = np.abs(emas[-1].double().cpu().numpy() - ref)
    worst = float((err / np.where(B > 0, B, 1.0)).max())
    print(f"average after {STEPS} updates (warmup={warmup}): worst error {worst:.3f} of the accumulated bound; "
          f"largest bound {B.max():.3e}, {int((err > B).sum())} outside")
    assert not (err > B).any()
    assert float(np.abs(ref - start.double().cpu().numpy()).max()) > 1e2 * float(B.max()), "the average hardly moved: nothing shown"
    for k in range(STEPS):  # and every single update within the per-update bound
        EC.judge(f"update {k + 1}", emas[k], before[k], flats[k], ws[k])


# ------------------------------------------------------------------------------------------------ 3. / 4. / 8. the averaged weights
@pytest.mark.parametrize("size", ["S17", "bert"])
def test_plain_trajectory_averaged_logits_and_leaving(size):
    if size == "bert":  # condition 8: the trajectory on the BERT model (the DeBERTa one: test_trajectory_.. above)
        same_trajectory(run(size, ema_decay=DECAY), run(size))
    M, opt, _, _, flats, emas = run(size, ema_decay=DECAY)
    twin = run(size, ema_decay=DECAY)  # never enters the context
    m, eng = M.m, M.m.engine()
    feed, rows = feeds(M)
    fresh = fresh_averaged(size, opt)
    m.eval()
    with torch.no_grad():
        want = fresh(**M.db).logits.clone()
        raw = m(**M.db).logits.clone()
        v0 = eng.params_version
        with m.ema_weights() as inside:
            assert inside is m and opt.ema_open and eng.params_version > v0
            assert torch.equal(bits(eng.flat), bits(emas[-1])) and torch.equal(bits(opt._ema), bits(flats[-1]))
            got = m(**M.db).logits.clone()
            with m.weights_frozen():
                got_frozen = m(**M.db).logits.clone()
            exported = opt.ema_state_dict()  # (inside the context too: the average, not the raw parameters)
        assert not opt.ema_open and eng.params_version > v0 + 1
        after = m(**M.db).logits.clone()
    assert torch.equal(got, want) and torch.equal(got_frozen, want), "averaged logits are not those of the fresh averaged model"
    assert not torch.equal(got, raw), "the averaged logits are the raw ones"
    assert torch.equal(after, raw), "the logits after leaving are not those before entering"
    for n, v in opt.ema_state_dict().items():
        assert torch.equal(bits(v), bits(exported[n])), n
    # ---- the same through a captured inference graph: captured on the raw weights, replayed on the average, then raw again
    if size != "bert":  # (the BERT model accepts the switch and runs eagerly)
        fresh.inference_graphs = m.inference_graphs = True
        with torch.no_grad():
            want_g = fresh(logit_rows=rows, **feed)["logits"].clone()
            raw_g = m(logit_rows=rows, **feed)["logits"].clone()
            assert m.__dict__.get("_graph_cache") and fresh.__dict__.get("_graph_cache")
            with m.ema_weights():
                got_g = m(logit_rows=rows, **feed)["logits"].clone()
            after_g = m(logit_rows=rows, **feed)["logits"].clone()
        m.inference_graphs = fresh.inference_graphs = False
        # the captured graphs are released here, with the device idle, and not by a collection in the middle of a later test
        from frozenbilm_amd import train_graph as TG

        torch.cuda.synchronize()
        TG.reset(m, TG.INFERENCE)
        TG.reset(fresh, TG.INFERENCE)
        assert not m.__dict__.get("_graph_cache") and not fresh.__dict__.get("_graph_cache")
        assert torch.equal(got_g, want_g) and not torch.equal(got_g, raw_g) and torch.equal(after_g, raw_g)
    # ---- 4. every bit is back, and the next step is the twin's
    assert torch.equal(bits(eng.flat), bits(flats[-1])) and torch.equal(bits(opt._ema), bits(emas[-1]))
    for n, p in m.named_parameters():
        assert torch.equal(bits(p), bits(twin[0].named[n])), n
    a, b = train(M, opt, first=STEPS, steps=1), train(twin[0], twin[1], first=STEPS, steps=1)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(bits(a[1][0]), bits(b[1][0])) and torch.equal(bits(a[2][0]), bits(b[2][0]))
    assert torch.equal(bits(opt._m), bits(twin[1]._m)) and torch.equal(bits(opt._v), bits(twin[1]._v))
    assert opt.ema_updates == twin[1].ema_updates == STEPS + 1


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_inside_the_context():
    M, opt, _, _, flats, emas = ema_run("S17")
    m = M.m
    sd_opt = opt.state_dict()
    sd_model = {k: v.clone() for k, v in m.state_dict().items()}
    with m.ema_weights():
        for what in (lambda: opt.step(), lambda: opt.step(clip_max_norm=1.0), m.ema_weights, opt.ema_weights, opt.state_dict,
                     lambda: opt.load_state_dict(sd_opt), lambda: m.load_state_dict(sd_model), m.merge_lora):
            with pytest.raises(RuntimeError, match="ema_weights"):
                what()
        assert opt.ema_open and torch.equal(bits(m.engine().flat), bits(emas[-1]))  # a refusal leaves the context as it was
    assert not opt.ema_open and torch.equal(bits(m.engine().flat), bits(flats[-1])) and torch.equal(bits(opt._ema), bits(emas[-1]))
    try:  # an exception inside the context: the weights are swapped back all the same
        with m.ema_weights():
            raise KeyError("x")
    except KeyError:
        pass
    assert not opt.ema_open and torch.equal(bits(m.engine().flat), bits(flats[-1]))
    assert set(opt.state_dict()) == {"state", "param_groups", "fbl_ema"}  # and outside everything works again
    with pytest.raises(RuntimeError):  # an optimizer without an average
        Model("S17").m.ema_weights()


def test_merge_lora_is_refused_inside_the_context():
    from oracle import deberta_oracle as O
    from tests import test_gpu_lora_model as TL

    cfg = TL._cfg()
    base = dict(cfg=cfg, P=O.synth_params(cfg, seed=51, std=0.05, ln_jitter=0.1))
    m, _ = TL._lora_model(base)
    batch = TL.to_dev(TL.synth_batch(cfg, B=3, L=14, seed=11))
    opt = FusedAdam(m, lr=1e-2, ema_decay=DECAY)
    m(**batch).loss.backward()
    opt.step()
    w_name = m.lora_names()[0] + ".weight"
    w0 = m.get_param(w_name).detach().clone()
    with m.ema_weights():
        with pytest.raises(RuntimeError, match="merge_lora"):
            m.merge_lora()
    assert torch.equal(m.get_param(w_name), w0), "the refused merge wrote the frozen master"
    assert any(".lora_B." in n for n in opt.ema_state_dict())  # the LoRA pair is averaged like every trainable parameter
    m.merge_lora()  # outside the context it goes through
    assert not torch.equal(m.get_param(w_name), w0)


# ------------------------------------------------------------------------------------------------ 6. checkpoints
def test_checkpoint_round_trip(tmp_path):
    from frozenbilm_amd.util.checkpoint import load_checkpoint, save_checkpoint

    M, opt, _, _, flats, emas = run("S17", kind="groups", ema_decay=DECAY, ema_warmup=True)
    m = M.m
    args = SimpleNamespace(lr=LR)
    raw_path, avg_path = str(tmp_path / "raw.pth"), str(tmp_path / "avg.pth")
    save_checkpoint(m, opt, 3, args, raw_path)
    save_checkpoint(m, opt, 3, args, avg_path, ema_weights=True)
    assert not opt.ema_open and torch.equal(bits(m.engine().flat), bits(flats[-1]))
    ck = torch.load(raw_path, map_location="cpu", weights_only=False)
    rec = ck["optimizer"]["fbl_ema"]
    assert set(ck["optimizer"]) == {"state", "param_groups", "fbl_ema"} and set(rec) == {"decay", "warmup", "updates", "params"}
    assert (rec["decay"], rec["warmup"], rec["updates"]) == (DECAY, True, STEPS)
    sl = opt._slices(m.engine())
    assert sorted(rec["params"]) == list(range(len(sl))) == sorted(ck["optimizer"]["state"])
    avg = opt.ema_state_dict()
    for i, (_, _, shape, name) in enumerate(sl):
        assert tuple(rec["params"][i].shape) == shape and torch.equal(rec["params"][i], avg[name].cpu()), name
    # ---- ema_weights=True: the "model" entry is the averaged model, the optimizer entry the same raw trajectory
    ck_avg = torch.load(avg_path, map_location="cpu", weights_only=False)
    assert ck_avg["model"].keys() == ck["model"].keys()
    n_avg = 0
    for k, v in ck_avg["model"].items():
        if k in avg:
            n_avg += 1
            assert torch.equal(v, avg[k].cpu()), k
        else:
            assert torch.equal(v, ck["model"][k]), k
    assert n_avg == len(avg) and any(not torch.equal(ck_avg["model"][k], ck["model"][k]) for k in avg)
    for i in rec["params"]:
        assert torch.equal(ck_avg["optimizer"]["fbl_ema"]["params"][i], rec["params"][i])
        assert torch.equal(ck_avg["optimizer"]["state"][i]["exp_avg"], ck["optimizer"]["state"][i]["exp_avg"])
    # ---- into a fresh model and optimizer with EMA on: the average, ema_updates and the next step
    N = Model("S17")
    nopt = optimizer(N, "groups", ema_decay=DECAY, ema_warmup=True)
    load_checkpoint(N.m, raw_path, optimizer=nopt, resume=True)
    assert nopt.ema_updates == STEPS and nopt.has_ema
    for n, v in nopt.ema_state_dict().items():
        assert torch.equal(bits(v), bits(avg[n])), n
    a, b = train(M, opt, first=STEPS, steps=1), train(N, nopt, first=STEPS, steps=1)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(bits(a[1][0]), bits(b[1][0])), "the resumed step differs"
    assert torch.equal(bits(a[2][0]), bits(b[2][0])) and nopt.ema_updates == opt.ema_updates == STEPS + 1
    # ---- the same file into torch.optim.Adam over the same parameters (it reads `state` and `param_groups` only) ...
    T = Model("S17")
    groups = [[p for p in g["params"]] for g in optimizer(T, "groups").param_groups]
    adam = torch.optim.Adam([dict(params=g) for g in groups], lr=LR, betas=BETAS)
    adam.load_state_dict(ck["optimizer"])
    assert len(adam.state) == len(sl) and all(int(st["step"]) == STEPS for st in adam.state.values())
    # ---- ... into a FusedAdam without EMA (the key is ignored) ...
    off = optimizer(T, "groups")
    off.load_state_dict(ck["optimizer"])
    assert not off.has_ema and off._step == STEPS and "fbl_ema" not in off.state_dict()
    # ---- ... a state without the key into EMA on: the average starts at the next step from the then-current parameters
    late = optimizer(T, "groups", ema_decay=DECAY)
    late.load_state_dict({k: v for k, v in ck["optimizer"].items() if k != "fbl_ema"})
    assert not late.has_ema and late.ema_updates == 0 and late._step == STEPS
    p_then = T.m.engine().flat.clone()
    train(T, late, first=STEPS, steps=1)
    assert late.ema_updates == 1
    EC.judge("the late average's first update", late._ema, p_then, T.m.engine().flat, EC.weight(DECAY, 1))
    # ---- ... and a shape mismatch is a ValueError
    bad = dict(ck["optimizer"], fbl_ema=dict(rec, params={**rec["params"], 0: rec["params"][0].reshape(-1)[:-1]}))
    with pytest.raises(ValueError):
        optimizer(Model("S17"), "groups", ema_decay=DECAY).load_state_dict(bad)


# ------------------------------------------------------------------------------------------------ 7. the loops
def test_main_evaluate_on_the_average():
    from frozenbilm_amd import main as P_main
    from tests.downstream_fixtures import Args, ListLoader, StubTokenizer, make_videotext_batches

    M, opt, _, _, flats, emas = ema_run("S17")
    m = M.m
    c = m.config
    tok = StubTokenizer(c.vocab_size)
    batches = make_videotext_batches(c.vocab_size, m.max_feats, m.features_dim, 2, 3, seed=31)
    fresh = fresh_averaged("S17", opt)

    def evaluate(model, **kw):
        torch.manual_seed(7)  # (the loop draws its masked tokens on the host)
        return P_main.evaluate(model, tok, ListLoader(batches), torch.device(DEV), Args(max_feats=m.max_feats, **kw))

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        want, raw, got = evaluate(fresh), evaluate(m), evaluate(m, eval_ema=True)
    assert got == want, (got, want)
    assert got["loss"] != raw["loss"], "evaluating on the average gave the raw weights' loss"
    assert not opt.ema_open and torch.equal(bits(m.engine().flat), bits(flats[-1])) and torch.equal(bits(opt._ema), bits(emas[-1]))
    assert evaluate(m) == raw
