"""GPU: deep prompt tuning (DebertaV2ForMaskedLM(..., n_prompt=P, prompt_depth=D)) through the model.

Shapes: the tiny model of tests/test_gpu_input_grads.py (vocab 512, H = 128, 2 heads, 3 layers, F = 32, the convolution behind
layer 0), B = 3 with ragged lengths (sample 1 has fewer frames, the last sample short right-padded text, so packed rows drop
rows), T in {0, 3}, L = 6, P in {1, 4}, D in {2, 3}: D = 2 overwrites the ConvLayer's output, D = 3 = num_hidden_layers also the
key/value stream of the enhanced mask decoder.

The oracle is not edited: tests/prompt_layers_refs.py swaps wrappers in for its `layer` and `emd` that rebuild the overwritten
input by torch.cat around leaf tensors (checked against the unwrapped oracle on the CPU, tests/test_prompt_layers_host.py); the
layer-0 prompt enters as extra rows of the looked-up table, as in tests/test_gpu_prompt_model.py.

Bounds, each that of the existing test of the same comparison: 2 % relative Frobenius against the bf16-operand oracle (BOUND of
test_gpu_input_grads.py), 2e-3 on logits / 1e-4 on gradients rows route against full logits, 2e-2 / 3e-2 decoder_rows on against
off (test_gpu_prompt_model.py); packed rows against the padded grid: equal logit bits on the requested rows and 3e-7 relative
Frobenius on the gradients (measured 6e-8 .. 9e-8); bit equality where the launch sequence is the same on the same bits
(prompt_depth = 1 against today's model, the compact-backward switch, the graph switches, a frozen prompt's neighbours)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.prompt_layers_refs import deep_prompts  # noqa: E402
from tests.test_gpu_input_grads import BOUND, E_NAME, _batch, _cfg, _dev, _gates_of, _oracle, _params, _rel_fro, _trainable  # noqa: E402
from tests.test_gpu_prompt_model import NAME, grads, worst_rel  # noqa: E402

DEV = "cuda"
B, LT, NL = 3, 6, 3
CASES = [pytest.param(T, P, D, id=f"T{T}-P{P}-D{D}") for T in (0, 3) for P in (1, 4) for D in (2, NL)]
NO_DEPTH = object()


def lname(i):
    return f"deberta.encoder.layer.{i}.prompt.weight"


def build(cfg, Pd, n_prompt, depth=NO_DEPTH, train=False, seed=5, **more):
    from frozenbilm_amd.model.config import DebertaV2Config
    from frozenbilm_amd.model.deberta import DebertaV2ForMaskedLM

    c = DebertaV2Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        max_position_embeddings=cfg.max_position_embeddings, position_buckets=cfg.position_buckets,
                        layer_norm_eps=cfg.layer_norm_eps, conv_kernel_size=cfg.conv_kernel_size)
    assert c.num_hidden_layers == NL
    torch.manual_seed(seed)  # (the dropout stream of a model is salted with the torch seed at its first training forward)
    kw = dict(more) if depth is NO_DEPTH else dict(more, prompt_depth=depth)
    m = DebertaV2ForMaskedLM(c, max_feats=cfg.max_feats, features_dim=cfg.features_dim, ds_factor_attn=cfg.ds_factor_attn,
                             ds_factor_ff=cfg.ds_factor_ff, n_ans=cfg.n_ans, n_prompt=n_prompt, **kw)
    layer_names = [lname(i) for i in range(1, m.prompt_depth)]
    missing, unexpected = m.load_state_dict(Pd, strict=False)
    assert not unexpected and all("position_ids" in k or k == NAME or k in layer_names or ".lora_" in k for k in missing), (missing, unexpected)
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():
        if n_prompt:  # as large as the word embeddings of the synthetic parameters
            m.get_param(NAME).copy_(torch.randn(n_prompt, cfg.hidden_size, generator=g) * 0.05)
        for n in layer_names:  # as large as the hidden rows they stand in for (LayerNorm outputs)
            m.get_param(n).copy_(torch.randn(n_prompt, cfg.hidden_size, generator=g) * 0.5)
    m.to(DEV)
    return m.train(train)


def feed(cfg, T, seed, labels=True):
    b = _batch(cfg, T, LT, seed=seed, B=B, labels=labels)
    if not T:
        b.pop("video"), b.pop("video_mask")
    return b


def text_rows(T, Pn, col=1):
    S = T + Pn + LT
    return torch.tensor([b * S + T + Pn + col for b in range(B)], device=DEV), S


def _downstream(T, Pn, D, seed, train=False):
    cfg = _cfg(T, n_ans=24)
    A = build(cfg, _params(cfg, seed), Pn, D, train)
    db = _dev(feed(cfg, T, seed=seed, labels=False))
    Wr = torch.randn(B, cfg.n_ans, generator=torch.Generator().manual_seed(4)).to(DEV)
    return cfg, A, db, Wr


def _step(m, db, seed=0):
    m.zero_grad(set_to_none=True)
    m.step_seed = seed
    out = m(**db)
    out.loss.backward()
    return out


# ------------------------------------------------------------------------------------------------ 1. prompt_depth = 1
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_depth_one_is_the_model_built_without_the_argument(train):
    T, Pn = 3, 4
    cfg = _cfg(T)
    Pd = _params(cfg, 61)
    db = _dev(feed(cfg, T, seed=41))
    base, one = build(cfg, Pd, Pn, NO_DEPTH, train), build(cfg, Pd, Pn, 1, train)
    assert [n for n, _ in one.named_parameters()] == [n for n, _ in base.named_parameters()]
    assert one.engine().offsets == base.engine().offsets and one.engine().order == base.engine().order
    oa, ob = _step(base, db, seed=3), _step(one, db, seed=3)
    if train:
        assert oa._run.p_hid > 0 and oa._run.seed_base == ob._run.seed_base != 0
    assert oa._run._site == ob._run._site
    assert torch.equal(oa.loss.detach(), ob.loss.detach()) and torch.equal(oa.logits.detach(), ob.logits.detach())
    ga, gb = grads(base), grads(one)
    assert set(ga) == set(gb) and all(torch.equal(ga[n], gb[n]) for n in ga)
    assert torch.equal(base.engine().flat_grad, one.engine().flat_grad)


# ------------------------------------------------------------------------------------------------ 2. what the layers read
@pytest.mark.parametrize("T,Pn,D", CASES)
def test_hidden_states_hold_the_parameters_bits_in_the_slots(T, Pn, D):
    cfg = _cfg(T)
    A = build(cfg, _params(cfg, 62), Pn, D)
    db = _dev(feed(cfg, T, seed=42, labels=False))
    S = T + Pn + LT
    params = [A.get_param(NAME).detach()] + [A.get_param(lname(i)).detach() for i in range(1, D)]
    for packed in (False, True):
        A.packed_rows = packed
        with torch.no_grad():
            kw = dict(logit_rows=text_rows(T, Pn)[0]) if packed else {}  # (packed rows serve calls on selected rows)
            out = A(**db, output_hidden_states=True, **kw)
        assert (out._run.pk is not None) == packed
        hs = out.hidden_states
        assert len(hs) == NL + 1 and all(h.shape == (B, S, cfg.hidden_size) for h in hs)
        for i in range(NL + 1):
            slots = hs[i][:, T:T + Pn]
            if 1 <= i < D:  # every sample reads the raw fp32 parameter: no LayerNorm, no mask multiply, no dropout
                w = A.get_param(lname(i)).detach()
                assert all(torch.equal(slots[b].view(torch.int32), w.view(torch.int32)) for b in range(B)), i
            else:  # an ordinary position: what the stage below computed
                assert all(not torch.equal(slots[b], w) for b in range(B) for w in params), i
                assert bool(torch.isfinite(slots).all())


# ------------------------------------------------------------------------------------------------ 3. the CPU oracle
@pytest.mark.parametrize("T,Pn,D", CASES)
def test_deep_prompt_gradients_vs_oracle(T, Pn, D):
    cfg = _cfg(T, n_ans=24)
    V, S = cfg.vocab_size, T + Pn + LT
    Pd = _params(cfg, 63)
    batch = feed(cfg, T, seed=43, labels=True)
    A = build(cfg, Pd, Pn, D)
    Wl = torch.randn(B, S, cfg.n_ans, generator=torch.Generator().manual_seed(3)) / (B * S)
    out = A(**_dev(batch), mlm=True)  # the MLM loss on the vocabulary ...
    gates = _gates_of(out._run, cfg)
    out.loss.backward()
    loss_gpu = out.loss.item()
    g_loss = grads(A)
    A.zero_grad(set_to_none=True)
    nolab = {k: v for k, v in batch.items() if k != "labels"}
    out2 = A(**_dev(nolab))  # ... and a downstream scalar on the answer logits of every row
    gates2 = _gates_of(out2._run, cfg)
    (out2.logits * Wl.to(DEV)).sum().backward()
    g_down = grads(A)
    # the oracle: the layer-0 prompt as rows V .. V+Pn-1 of the looked-up table, Pn ids in front of the text; the layers' prompts
    # through the wrappers
    Po = dict(Pd)
    Po[E_NAME] = torch.cat([Pd[E_NAME].detach(), A.get_param(NAME).detach().cpu()], 0)
    hb = "lm_predictions.lm_head.bias"  # (the MLM head reads the same table: its bias grows by Pn entries that nothing reads)
    Po[hb] = torch.cat([Pd[hb].detach(), torch.zeros(Pn)])
    ob = dict(nolab)
    ob["input_ids"] = torch.cat([(V + torch.arange(Pn)).expand(B, -1), batch["input_ids"]], 1)
    ob["attention_mask"] = torch.cat([torch.ones(B, Pn, dtype=torch.long), batch["attention_mask"]], 1)
    lab = torch.cat([torch.full((B, Pn), -100, dtype=torch.long), batch["labels"]], 1)

    def reference(kind):
        _trainable(Po, extra=(E_NAME,))
        leaves = {i: A.get_param(lname(i)).detach().cpu().clone().requires_grad_() for i in range(1, D)}
        with deep_prompts(leaves, T, NL):
            if kind == "loss":
                ref = _oracle(Po, cfg, {**ob, "labels": lab}, gates, B, mlm=True)
                # (the extended table is the MLM head's too: its extra columns are no words; keep them out of the softmax)
                lg = ref["logits"][..., :V]
                full = torch.cat([torch.full((B, T), -100, dtype=torch.long), lab], 1) if T else lab
                scalar = torch.nn.functional.cross_entropy(lg.reshape(-1, V), full.reshape(-1), ignore_index=-100)
            else:
                ref = _oracle(Po, cfg, ob, gates2, B)
                scalar = (ref["logits"] * Wl).sum()
        scalar.backward()
        return ref, scalar, leaves

    for kind, got, gpu_out in (("loss", g_loss, out), ("downstream", g_down, out2)):
        ref, scalar, leaves = reference(kind)
        if kind == "loss":
            assert abs(loss_gpu - scalar.item()) < 5e-3, (loss_gpu, scalar.item())
        else:
            assert (gpu_out.logits.detach().float().cpu() - ref["logits"].detach()).abs().max().item() < 5e-2
        rp = _rel_fro(got[NAME].float().cpu(), Po[E_NAME].grad[V:])
        rl = {i: _rel_fro(got[lname(i)].float().cpu(), leaves[i].grad) for i in leaves}
        worst = 0.0, ""
        for n, g in got.items():
            if n == NAME or n in {lname(i) for i in leaves}:
                continue
            r = Po[n].grad if Po[n].grad is not None else torch.zeros_like(Po[n])
            d = (g.float().cpu() - r).norm().item()
            worst = max(worst, (d / max(r.norm().item(), 1e-12) if d else 0.0, n))
        print(f"[oracle {kind} T={T} P={Pn} D={D}] layer-0 prompt {rp:.5f}; layer prompts {({i: round(v, 5) for i, v in rl.items()})}; "
              f"worst trainable {worst}")
        assert all(leaves[i].grad.norm().item() > 0 for i in leaves)
        assert rp < BOUND, rp
        assert all(v < BOUND for v in rl.values()), rl
        assert worst[0] < BOUND, worst


# ------------------------------------------------------------------------------------------------ 4. routes
@pytest.mark.parametrize("T,Pn,D", CASES)
def test_logit_rows_against_full_logits(T, Pn, D):
    cfg, A, db, Wr = _downstream(T, Pn, D, 64)
    rows, S = text_rows(T, Pn)
    full = A(**db).logits
    (full.reshape(B * S, -1)[rows] * Wr).sum().backward()
    ref = grads(A)
    A.zero_grad(set_to_none=True)
    lr = A(**db, logit_rows=rows).logits
    (lr * Wr).sum().backward()
    d, worst = (lr.detach() - full.detach().reshape(B * S, -1)[rows]).abs().max().item(), worst_rel(grads(A), ref)
    print(f"[rows vs full T={T} P={Pn} D={D}] logits max-abs diff {d:.3g}, worst gradient Frobenius diff {worst:.3g}")
    assert all(ref[lname(i)].norm().item() > 0 for i in range(1, D))
    assert d < 2e-3 and worst < 1e-4


@pytest.mark.parametrize("T,Pn,D", CASES)
def test_packed_rows_against_the_padded_grid(T, Pn, D):
    cfg, A, db, Wr = _downstream(T, Pn, D, 65)
    rows, S = text_rows(T, Pn)
    res = {}
    for packed in (False, True):
        A.packed_rows = packed
        A.zero_grad(set_to_none=True)
        out = A(**db, logit_rows=rows)
        run = out._run
        if packed:  # the last sample's padding is gone, its prompt slots are not
            assert run.pk is not None and run.N == run.pk.n < B * S
            assert int(run.pk.row0[-1] - run.pk.row0[-2]) >= T + Pn
        else:
            assert run.pk is None
        (out.logits * Wr).sum().backward()
        res[packed] = (out.logits.detach().clone(), grads(A))
    d, worst = (res[True][0] - res[False][0]).abs().max().item(), worst_rel(res[True][1], res[False][1])
    print(f"[packed vs grid T={T} P={Pn} D={D}] logits max-abs diff {d:.3g} (bits equal: {torch.equal(res[True][0], res[False][0])}), "
          f"worst gradient Frobenius diff {worst:.3g}")
    assert all(res[False][1][lname(i)].norm().item() > 0 for i in range(1, D))
    # rows that exist are computed by the same kernels on the same values: the logits keep their bits; the gradients differ by
    # the order of fp32 sums over rows only
    assert torch.equal(res[True][0], res[False][0]) and worst < 3e-7


@pytest.mark.parametrize("packed", [False, True], ids=["grid", "packed"])
@pytest.mark.parametrize("T,Pn,D", CASES)
def test_decoder_rows_against_the_full_decoder(T, Pn, D, packed):
    cfg, A, db, Wr = _downstream(T, Pn, D, 66)
    rows, S = text_rows(T, Pn)
    A.packed_rows = packed
    res = {}
    for on in (False, True):
        A.decoder_rows = on
        A.zero_grad(set_to_none=True)
        out = A(**db, logit_rows=rows)
        assert (out._run.dec_grid is not None) == on and (out._run.pk is not None) == packed
        (out.logits * Wr).sum().backward()
        res[on] = (out.logits.detach().clone(), grads(A))
    d, worst = (res[True][0] - res[False][0]).abs().max().item(), worst_rel(res[True][1], res[False][1])
    print(f"[decoder_rows on vs off T={T} P={Pn} D={D} packed={packed}] logits max-abs diff {d:.3g}, "
          f"worst gradient Frobenius diff {worst:.3g}")
    assert all(res[False][1][lname(i)].norm().item() > 0 for i in range(1, D))
    assert d < 2e-2 and worst < 3e-2


@pytest.mark.parametrize("T,Pn,D", CASES)
def test_compact_backward_switch_against_the_padded_backward(T, Pn, D):
    """a model with prompt slots keeps the padded backward (Engine._backward_rows); the switch changes no bit"""
    cfg = _cfg(T)
    A = build(cfg, _params(cfg, 67), Pn, D, train=True)
    db = _dev(feed(cfg, T, seed=47))
    res = {}
    for force in (False, True):
        A.compact_backward = force
        out = _step(A, db, seed=2)
        res[force] = (out.loss.detach().clone(), grads(A), out._run.bwd_compact)
    assert torch.equal(res[True][0], res[False][0])
    assert res[True][1].keys() == res[False][1].keys()
    assert all(torch.equal(res[True][1][n], res[False][1][n]) for n in res[False][1])
    assert all(res[False][1][lname(i)].norm().item() > 0 for i in range(1, D))
    assert not res[False][2]


def test_graph_switches_leave_a_deep_prompt_model_eager():
    from frozenbilm_amd import train_graph as TG

    T, Pn, D = 3, 4, NL
    cfg = _cfg(T, n_ans=24)
    A = build(cfg, _params(cfg, 68), Pn, D, train=True)
    db = _dev(feed(cfg, T, seed=48))
    nolab = {k: v for k, v in db.items() if k != "labels"}
    rows, S = text_rows(T, Pn)

    def calls():
        got = []
        A.train()
        A.zero_grad(set_to_none=True)
        A.step_seed = 0
        out = A(**db, mlm=True)  # the training_graphs route's call
        out.loss.backward()
        got += [out.loss.detach().clone()] + list(grads(A).values())
        A.zero_grad(set_to_none=True)
        A.step_seed = 0
        lg = A(**nolab, logit_rows=rows).logits  # the finetune_graphs route's call
        lg.sum().backward()
        got += [lg.detach().clone()] + list(grads(A).values())
        A.eval()
        with torch.no_grad():  # the inference_graphs route's call
            got.append(A(**nolab, logit_rows=rows).logits.clone())
        return got

    eager = calls()
    A.inference_graphs = A.training_graphs = A.finetune_graphs = True
    graphed = calls()
    assert len(eager) == len(graphed) and all(torch.equal(a, b) for a, b in zip(eager, graphed))
    for route in TG.ROUTES:
        st = TG.stats(A, route)
        assert st.captures == 0 and st.replays == 0 and not A.__dict__.get(route.cache), route.switch


def test_lora_and_inputs_embeds_on_a_deep_prompt_model():
    """LoRA on the projections that read the overwritten rows, and inputs_embeds = E[ids] in place of the ids: the same launches
    on the same bits, so loss and every gradient are bit-identical between the two calls; the LoRA factors that can have a
    gradient at initialisation (B = 0: lora_B) and every layer prompt have one"""
    T, Pn, D = 3, 4, NL
    cfg = _cfg(T)
    A = build(cfg, _params(cfg, 72), Pn, D, train=True, lora_rank=4)
    db = _dev(feed(cfg, T, seed=52))
    out = _step(A, db, seed=1)
    loss, ref = out.loss.detach().clone(), grads(A)
    assert all(ref[lname(i)].norm().item() > 0 for i in range(1, D))
    lb = [n for n in ref if n.endswith(".lora_B.weight")]
    assert len(lb) == 2 * NL and all(ref[n].norm().item() > 0 and bool(torch.isfinite(ref[n]).all()) for n in lb)
    kw = dict(db)
    e = A.get_param(E_NAME).detach()[kw.pop("input_ids")].clone().requires_grad_()
    A.zero_grad(set_to_none=True)
    A.step_seed = 1
    out = A(**kw, inputs_embeds=e)
    out.loss.backward()
    assert torch.equal(out.loss.detach(), loss)
    got = grads(A)
    assert got.keys() == ref.keys() and all(torch.equal(got[n], ref[n]) for n in ref)
    assert e.grad is not None and e.grad.shape == (B, LT, cfg.hidden_size) and float(e.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 5. freezing
@pytest.mark.parametrize("T,Pn,D", CASES)
def test_freezing_a_layer_prompt(T, Pn, D):
    """layer k's prompt frozen: no .grad, its value and Adam moments keep their bits over two FusedAdam steps, every live gradient
    is the full step's bit for bit (the slots' rows of the stream gradient are cleared all the same)"""
    from frozenbilm_amd.optim import FusedAdam

    cfg = _cfg(T)
    A = build(cfg, _params(cfg, 69), Pn, D, train=True)
    db = _dev(feed(cfg, T, seed=49))
    k = D - 1
    name = lname(k)
    prompt = A.get_param(name)
    opt = FusedAdam(A, lr=1e-2)
    idx = [id(p) for g in opt.param_groups for p in g["params"]].index(id(prompt))
    _step(A, db, seed=0)
    opt.step(clip_max_norm=1.0)  # a live step first: its Adam moments exist
    st = opt.state_dict()["state"][idx]
    m0, v0 = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    assert m0.norm().item() > 0 and tuple(m0.shape) == (Pn, cfg.hidden_size)
    out = _step(A, db, seed=1)
    loss, logits, live = out.loss.detach().clone(), out.logits.detach().clone(), grads(A)
    assert live[name].norm().item() > 0
    prompt.requires_grad_(False)
    out = _step(A, db, seed=1)
    assert prompt.grad is None
    assert torch.equal(loss, out.loss.detach()) and torch.equal(logits, out.logits.detach())
    frozen = grads(A)
    assert set(frozen) == set(live) - {name}
    for n in frozen:
        assert torch.equal(frozen[n], live[n]), n
    before = prompt.detach().clone()
    other = A.get_param(f"deberta.encoder.layer.{k}.output.LayerNorm.weight")
    other_before = other.detach().clone()
    for i in range(2):
        _step(A, db, seed=2 + i)
        opt.step(clip_max_norm=1.0)
    st = opt.state_dict()["state"][idx]
    assert torch.equal(prompt.detach(), before) and not torch.equal(other.detach(), other_before)
    assert torch.equal(st["exp_avg"], m0) and torch.equal(st["exp_avg_sq"], v0)
    prompt.requires_grad_(True)  # live again: it moves
    _step(A, db, seed=4)
    opt.step(clip_max_norm=1.0)
    assert not torch.equal(prompt.detach(), before) and bool(torch.isfinite(prompt).all())


@pytest.mark.parametrize("T,Pn,D", CASES)
def test_backward_stops_below_the_lowest_live_layer_prompt(T, Pn, D):
    """everything below layer 1 frozen (the embedding stage, layer 0, the convolution, the LayerNorm over the position table,
    whose stage is layer 0): the backward runs the stages from layer 1 up and launches nothing under it -- the forward saved
    nothing there -- and layer 1's prompt, the lowest live leaf, gets its gradient"""
    cfg = _cfg(T)
    A = build(cfg, _params(cfg, 70), Pn, D, train=False)
    db = _dev(feed(cfg, T, seed=50))
    def step():  # (the backward consumes what the forward saved: counted in between)
        A.zero_grad(set_to_none=True)
        out = A(**db)
        saved = len(out._run.layers)
        out.loss.backward()
        return out._run, saved

    _, saved_full = step()
    full = grads(A)
    from frozenbilm_amd.live_set import stage_of

    stages = A.engine().plan().stages
    low = stages.index("layer1")
    dead = [n for n in A.trainable_names() if stages.index(stage_of(n, NL)) < low]
    assert NAME in dead and lname(1) not in dead and any("layer.0." in n for n in dead)
    for n in dead:
        A.get_param(n).requires_grad_(False)
    run, saved = step()
    assert run.plan.running[0] == "layer1" and not run.plan.runs("conv") and not run.plan.runs("layer0") and not run.plan.runs("emb")
    assert saved_full == NL + 1 and saved == NL  # layer 1 and the two decoder passes; layer 0 was not saved
    assert run.conv_norm is None and run.emb_norm is None
    assert all(A.get_param(n).grad is None for n in dead)
    part = grads(A)
    assert set(part) == set(full) - set(dead)
    rel = {n: _rel_fro(part[n].float().cpu(), full[n].float().cpu()) for n in part}
    print(f"[lowest stage layer1 T={T} P={Pn} D={D}] layer-1 prompt against the all-live step: rel Frobenius {rel[lname(1)]:.3g}; "
          f"worst {max(rel.values()):.3g}")
    assert part[lname(1)].norm().item() > 0
    assert max(rel.values()) < BOUND  # (with dead leaves below, GEMMs may take other routes: bf16-operand agreement, not bits)


# ------------------------------------------------------------------------------------------------ 6. gradients on hidden states
@pytest.mark.parametrize("T,Pn,D", CASES)
def test_gradient_on_a_slot_row_of_hidden_states_reaches_the_layer_prompt_only(T, Pn, D):
    cfg = _cfg(T)
    S, H = T + Pn + LT, cfg.hidden_size
    A = build(cfg, _params(cfg, 71), Pn, D)
    db = _dev(feed(cfg, T, seed=51, labels=False))
    g8 = torch.Generator().manual_seed(8)  # magnitudes over a few binades: the order of the adds shows in the last bits
    W = torch.randn(B, Pn, H, generator=g8) * torch.exp2(torch.randint(-4, 5, (B, 1, 1), generator=g8).float())
    for i in range(1, D):
        A.zero_grad(set_to_none=True)
        hs = A(**db, output_hidden_states=True).hidden_states
        assert hs[i].requires_grad
        (hs[i][:, T:T + Pn] * W.to(DEV)).sum().backward()
        acc = torch.zeros(Pn, H)
        for b in range(B):  # the ascending-b fp32 sum, from the zero the buffer holds
            acc += W[b]
        got = grads(A)
        assert torch.equal(got[lname(i)].cpu(), acc), i
        # nowhere upstream: the stages below layer i, the other layers' prompts included, receive exactly zero
        from frozenbilm_amd.live_set import stage_of

        stages = A.engine().plan().stages
        at = stages.index(stage_of(lname(i), NL))
        for n, g in got.items():
            if n != lname(i) and stages.index(stage_of(n, NL)) < at and not n.startswith("deberta.encoder.LayerNorm."):
                assert float(g.abs().max()) == 0.0, (i, n)
        # a row outside the slots does flow upstream
        A.zero_grad(set_to_none=True)
        hs = A(**db, output_hidden_states=True).hidden_states
        hs[i][:, T + Pn:].sum().backward()
        got = grads(A)
        assert float(got[lname(i)].abs().max()) == 0.0
        assert got["deberta.embeddings.LayerNorm.weight"].norm().item() > 0 and got[NAME].norm().item() > 0
