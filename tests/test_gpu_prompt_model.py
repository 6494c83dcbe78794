"""GPU: prompt tuning (DebertaV2ForMaskedLM(..., n_prompt=P)) through the model.

Model A carries the prompt; model B is the same weights with n_prompt = 0, fed the imitation a caller could build today:
inputs_embeds = cat([prompt.expand(B, -1, -1), E[ids]]), attention_mask / labels extended by ones / -100.  Only the embedding
stage differs between the two, and there only in WHO writes the fp32 rows in front of the LayerNorm (fbl_embed_assemble
against torch copies of the same values) and who sums the prompt slots' rows of dt0 (fbl_prompt_grad against the caller): every
output and every gradient both models have is the same launch sequence on the same bits, so bit equality is asserted
everywhere; reading Engine._backward_bottom shows no sum that the inputs_embeds route orders differently.

Shapes: the tiny model of tests/test_gpu_input_grads.py (vocab 512, H = 128, 2 heads, 3 layers, F = 32), B = 3, (T, L) in
{(2, 9), (0, 12)} (with video slots, and without a video at all), P in {1, 5}; sample 1 has fewer frames, the last sample short
right-padded text (so packed rows drop rows).

Bounds, each that of the existing test of the same comparison: 2 % relative Frobenius against the bf16-operand oracle
(test_gpu_input_grads.py), 2e-3 on logits / 1e-4 on gradients rows route against full logits (test_gpu_finetune_rows.py), 2e-2 /
3e-2 packed against padded and decoder_rows on against off (test_gpu_finetune_rows.py, test_gpu_decoder_rows.py).

The oracle has no inputs_embeds argument; the word-embedding table enters it only through the lookup (downstream mode: the
answer table is the head's), so the prompt is fed as P extra rows of that table addressed by P extra ids in front of the
text -- the same rows in front of the LayerNorm -- and the prompt's gradient is those rows of the table's gradient."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_input_grads import BOUND, E_NAME, _batch, _cfg, _dev, _gates_of, _oracle, _params, _rel_fro, _trainable  # noqa: E402

DEV = "cuda"
NAME = "deberta.embeddings.prompt_embeddings.weight"
B = 3
CASES = [pytest.param(T, Lt, P, id=f"T{T}-L{Lt}-P{P}") for T, Lt in ((2, 9), (0, 12)) for P in (1, 5)]


def build(cfg, Pd, n_prompt=0, train=False, seed=5):
    from frozenbilm_amd.model.config import DebertaV2Config
    from frozenbilm_amd.model.deberta import DebertaV2ForMaskedLM

    c = DebertaV2Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        max_position_embeddings=cfg.max_position_embeddings, position_buckets=cfg.position_buckets,
                        layer_norm_eps=cfg.layer_norm_eps, conv_kernel_size=cfg.conv_kernel_size)
    torch.manual_seed(seed)  # (the dropout stream of a model is salted with the torch seed at its first training forward)
    m = DebertaV2ForMaskedLM(c, max_feats=cfg.max_feats, features_dim=cfg.features_dim, ds_factor_attn=cfg.ds_factor_attn,
                             ds_factor_ff=cfg.ds_factor_ff, n_ans=cfg.n_ans, n_prompt=n_prompt)
    missing, unexpected = m.load_state_dict(Pd, strict=False)
    assert not unexpected and all("position_ids" in k or k == NAME for k in missing), (missing, unexpected)
    if n_prompt:  # as large as the word embeddings of the synthetic parameters
        with torch.no_grad():
            m.get_param(NAME).copy_(torch.randn(n_prompt, cfg.hidden_size, generator=torch.Generator().manual_seed(99)) * 0.05)
    m.to(DEV)
    return m.train(train)


def feed(cfg, T, Lt, seed, labels=True):
    b = _batch(cfg, T, Lt, seed=seed, B=B, labels=labels)
    if not T:
        b.pop("video"), b.pop("video_mask")
    return b


def imitation(mB, db, prompt):
    """the call a user of today's model would make: (kwargs, the inputs_embeds leaf)"""
    Pn = prompt.shape[0]
    kw = dict(db)
    ids = kw.pop("input_ids")
    E = mB.get_param(E_NAME).detach()
    e = torch.cat([prompt.detach().expand(B, -1, -1), E[ids]], 1).clone().requires_grad_()
    kw["inputs_embeds"] = e
    kw["attention_mask"] = torch.cat([torch.ones(B, Pn, dtype=torch.long, device=DEV), kw["attention_mask"]], 1)
    if "labels" in kw:
        kw["labels"] = torch.cat([torch.full((B, Pn), -100, dtype=torch.long, device=DEV), kw["labels"]], 1)
    return kw, e


def grads(m, skip=()):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad and n not in skip}


def worst_rel(got, ref):
    """worst relative Frobenius difference; a gradient that is exactly zero on both sides (linear_video without a video) counts 0"""
    assert got.keys() == ref.keys()
    w = 0.0
    for n in ref:
        d = (got[n].float() - ref[n].float()).norm().item()
        w = max(w, d / max(ref[n].float().norm().item(), 1e-12) if d else 0.0)
    return w


def text_rows(T, Pn, Lt, col=1):
    S = T + Pn + Lt
    return torch.tensor([b * S + T + Pn + col for b in range(B)], device=DEV), S


# ------------------------------------------------------------------------------------------------ 1. first-class = imitation
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("T,Lt,Pn", CASES)
def test_first_class_prompt_equals_its_imitation(T, Lt, Pn, train):
    cfg = _cfg(T)
    Pd = _params(cfg, 81)
    db = _dev(feed(cfg, T, Lt, seed=21))
    A, Bm = build(cfg, Pd, Pn, train), build(cfg, Pd, 0, train)
    prompt = A.get_param(NAME)
    S = T + Pn + Lt
    A.step_seed = Bm.step_seed = 3
    oa = A(**db)
    oa.loss.backward()
    kw, e = imitation(Bm, db, prompt)
    ob = Bm(**kw)
    ob.loss.backward()
    assert oa._run.S == ob._run.S == S and oa._run.P == Pn and ob._run.P == 0
    if train:
        assert oa._run.p_hid > 0 and oa._run.seed_base == ob._run.seed_base != 0
    assert oa.logits.shape == (B, S, cfg.vocab_size)
    assert torch.equal(oa.loss.detach(), ob.loss.detach())
    assert torch.equal(oa.logits.detach(), ob.logits.detach())
    ga, gb = grads(A), grads(Bm)
    assert set(ga) == set(gb) | {NAME}
    for n in gb:
        assert torch.equal(ga[n], gb[n]), n
    eg = e.grad.cpu()
    acc = torch.zeros(Pn, cfg.hidden_size)
    for b in range(B):  # the ascending-b fp32 sum
        acc += eg[b, :Pn]
    assert float(acc.abs().max()) > 0
    assert torch.equal(ga[NAME].cpu(), acc)
    # eval-mode logits without gradients, and with output_hidden_states: the prompt slots are rows like any other
    A.eval(), Bm.eval()
    with torch.no_grad():
        kw2 = {k: (v.detach() if k == "inputs_embeds" else v) for k, v in kw.items() if k != "labels"}
        nolab = {k: v for k, v in db.items() if k != "labels"}
        xa, xb = A(**nolab, output_hidden_states=True), Bm(**kw2, output_hidden_states=True)
        assert torch.equal(xa.logits, xb.logits)
        assert xa.hidden_states[0].shape == (B, S, cfg.hidden_size)
        assert all(torch.equal(h, k) for h, k in zip(xa.hidden_states, xb.hidden_states))


def test_inputs_embeds_on_a_prompt_model_and_the_position_limit():
    """the prompt sits in front of given embeddings too; the input gradient comes back for the text rows alone; a sequence that
    passes max_position_embeddings only through the prompt is refused by a message that names the prompt"""
    T, Lt, Pn = 2, 9, 5
    cfg = _cfg(T)
    Pd = _params(cfg, 82)
    db = _dev(feed(cfg, T, Lt, seed=22))
    A = build(cfg, Pd, Pn)
    E = A.get_param(E_NAME).detach()
    out0 = A(**db)
    out0.loss.backward()
    ref_loss, ref = out0.loss.detach().clone(), grads(A)
    A.zero_grad(set_to_none=True)
    kw = dict(db)
    e = E[kw.pop("input_ids")].clone().requires_grad_()
    out = A(**kw, inputs_embeds=e)
    out.loss.backward()
    assert torch.equal(out.loss.detach(), ref_loss)
    for n, g in grads(A).items():
        assert torch.equal(g, ref[n]), n
    assert e.grad.shape == (B, Lt, cfg.hidden_size) and float(e.grad.abs().max()) > 0
    assert float(e.grad[db["attention_mask"] == 0].abs().max()) == 0.0
    Lmax = cfg.max_position_embeddings - T - Pn + 1
    long_ids = torch.full((1, Lmax), 7, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError, match=f"prompt {Pn}"):
        A(input_ids=long_ids, video=db["video"][:1])


# ------------------------------------------------------------------------------------------------ 2. the CPU oracle
@pytest.mark.parametrize("T,Lt,Pn", CASES)
def test_prompt_gradient_vs_oracle(T, Lt, Pn):
    cfg = _cfg(T, n_ans=24)
    V, S = cfg.vocab_size, T + Pn + Lt
    Pd = _params(cfg, 83)
    batch = feed(cfg, T, Lt, seed=23, labels=False)
    A = build(cfg, Pd, Pn)
    Wl = torch.randn(B, S, cfg.n_ans, generator=torch.Generator().manual_seed(3)) / (B * S)
    out = A(**_dev(batch))
    gates = _gates_of(out._run, cfg)
    (out.logits * Wl.to(DEV)).sum().backward()
    # the oracle: the prompt as rows V .. V+Pn-1 of the looked-up table, Pn ids in front of the text
    Po = dict(Pd)
    Po[E_NAME] = torch.cat([Pd[E_NAME].detach(), A.get_param(NAME).detach().cpu()], 0)
    _trainable(Po, extra=(E_NAME,))
    ob = dict(batch)
    ob["input_ids"] = torch.cat([(V + torch.arange(Pn)).expand(B, -1), batch["input_ids"]], 1)
    ob["attention_mask"] = torch.cat([torch.ones(B, Pn, dtype=torch.long), batch["attention_mask"]], 1)
    ref = _oracle(Po, cfg, ob, gates, B)
    (ref["logits"] * Wl).sum().backward()
    assert (out.logits.detach().float().cpu() - ref["logits"].detach()).abs().max().item() < 5e-2
    gp = Po[E_NAME].grad[V:]
    assert gp.norm().item() > 0
    rp = _rel_fro(A.get_param(NAME).grad.float().cpu(), gp)
    worst = 0.0, ""
    for n, g in grads(A, skip=(NAME,)).items():
        r = Po[n].grad if Po[n].grad is not None else torch.zeros_like(Po[n])
        d = (g.float().cpu() - r).norm().item()
        worst = max(worst, (d / max(r.norm().item(), 1e-12) if d else 0.0, n))
    print(f"[oracle T={T} L={Lt} P={Pn}] prompt gradient rel Frobenius {rp:.5f}; worst trainable {worst}")
    assert rp < BOUND, rp
    assert worst[0] < BOUND, worst


# ------------------------------------------------------------------------------------------------ 3. routes
def _downstream(T, Lt, Pn, seed, train=False):
    cfg = _cfg(T, n_ans=24)
    A = build(cfg, _params(cfg, seed), Pn, train)
    db = _dev(feed(cfg, T, Lt, seed=seed, labels=False))
    Wr = torch.randn(B, cfg.n_ans, generator=torch.Generator().manual_seed(4)).to(DEV)
    return cfg, A, db, Wr


@pytest.mark.parametrize("T,Lt,Pn", CASES)
def test_logit_rows_against_full_logits(T, Lt, Pn):
    cfg, A, db, Wr = _downstream(T, Lt, Pn, 84)
    rows, S = text_rows(T, Pn, Lt)
    full = A(**db).logits
    (full.reshape(B * S, -1)[rows] * Wr).sum().backward()
    ref = grads(A)
    A.zero_grad(set_to_none=True)
    lr = A(**db, logit_rows=rows).logits
    (lr * Wr).sum().backward()
    d, worst = (lr.detach() - full.detach().reshape(B * S, -1)[rows]).abs().max().item(), worst_rel(grads(A), ref)
    print(f"[rows vs full T={T} L={Lt} P={Pn}] logits max-abs diff {d:.3g}, worst gradient Frobenius diff {worst:.3g}")
    assert ref[NAME].norm().item() > 0
    assert d < 2e-3 and worst < 1e-4


@pytest.mark.parametrize("T,Lt,Pn", CASES)
def test_packed_rows_against_the_padded_grid(T, Lt, Pn):
    cfg, A, db, Wr = _downstream(T, Lt, Pn, 85)
    rows, S = text_rows(T, Pn, Lt)
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
    print(f"[packed vs grid T={T} L={Lt} P={Pn}] logits max-abs diff {d:.3g}, worst gradient Frobenius diff {worst:.3g}")
    assert res[False][1][NAME].norm().item() > 0
    assert d < 2e-2 and worst < 3e-2


@pytest.mark.parametrize("packed", [False, True], ids=["grid", "packed"])
@pytest.mark.parametrize("T,Lt,Pn", CASES)
def test_decoder_rows_against_the_full_decoder(T, Lt, Pn, packed):
    cfg, A, db, Wr = _downstream(T, Lt, Pn, 86)
    rows, S = text_rows(T, Pn, Lt)
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
    print(f"[decoder_rows on vs off T={T} L={Lt} P={Pn} packed={packed}] logits max-abs diff {d:.3g}, "
          f"worst gradient Frobenius diff {worst:.3g}")
    assert res[False][1][NAME].norm().item() > 0
    assert d < 2e-2 and worst < 3e-2


# ------------------------------------------------------------------------------------------------ 4. graph switches
def test_graph_switches_leave_a_prompt_model_eager():
    from frozenbilm_amd import train_graph as TG

    T, Lt, Pn = 2, 9, 5
    cfg = _cfg(T, n_ans=24)
    A = build(cfg, _params(cfg, 87), Pn, train=True)
    db = _dev(feed(cfg, T, Lt, seed=27))
    nolab = {k: v for k, v in db.items() if k != "labels"}
    rows, S = text_rows(T, Pn, Lt)

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


# ------------------------------------------------------------------------------------------------ 5. freezing
def _step(m, db, seed=0):
    m.zero_grad(set_to_none=True)
    m.step_seed = seed
    out = m(**db)
    out.loss.backward()
    return out.loss.detach().clone(), out.logits.detach().clone()


@pytest.mark.parametrize("T,Lt,Pn", CASES)
def test_freezing_the_prompt(T, Lt, Pn):
    from frozenbilm_amd.optim import FusedAdam

    cfg = _cfg(T)
    A = build(cfg, _params(cfg, 88), Pn, train=True)
    db = _dev(feed(cfg, T, Lt, seed=28))
    prompt = A.get_param(NAME)
    loss, logits = _step(A, db)
    live = grads(A)
    assert live[NAME].norm().item() > 0
    # frozen: nothing is launched for it, every other output and gradient keeps its bits
    prompt.requires_grad_(False)
    loss_f, logits_f = _step(A, db)
    assert prompt.grad is None
    assert torch.equal(loss, loss_f) and torch.equal(logits, logits_f)
    frozen = grads(A)
    assert set(frozen) == set(live) - {NAME}
    for n in frozen:
        assert torch.equal(frozen[n], live[n]), n
    opt = FusedAdam(A, lr=1e-2)
    idx = [id(p) for g in opt.param_groups for p in g["params"]].index(id(prompt))
    before = prompt.detach().clone()
    other = A.get_param("deberta.embeddings.LayerNorm.weight")
    other_before = other.detach().clone()
    for i in range(3):
        _step(A, db, seed=i)
        opt.step(clip_max_norm=1.0)
    assert torch.equal(prompt.detach(), before) and not torch.equal(other.detach(), other_before)
    assert idx not in opt.state_dict()["state"]
    # live again: it moves, and its Adam state appears
    prompt.requires_grad_(True)
    _step(A, db, seed=3)
    assert prompt.grad is not None and prompt.grad.norm().item() > 0
    opt.step(clip_max_norm=1.0)
    assert not torch.equal(prompt.detach(), before) and bool(torch.isfinite(prompt).all())
    st = opt.state_dict()["state"]
    assert idx in st and tuple(st[idx]["exp_avg"].shape) == (Pn, cfg.hidden_size) and st[idx]["exp_avg"].norm().item() > 0
    # the prompt alone live: the embedding stage stays in the plan and fills its gradient
    for n, p in A.named_parameters():
        p.requires_grad_(n == NAME)
    A.eval()
    _step(A, db)
    only = prompt.grad.detach().clone()
    assert A.engine().plan().runs("emb") and A.engine().live_order == [NAME]
    assert all(p.grad is None for n, p in A.named_parameters() if n != NAME)
    for n in A.trainable_names():
        A.get_param(n).requires_grad_(True)
    _step(A, db)
    rel = _rel_fro(only.float().cpu(), prompt.grad.float().cpu())
    print(f"[prompt alone live T={T} L={Lt} P={Pn}] its gradient against the all-live step: rel Frobenius {rel:.3g}")
    assert only.norm().item() > 0 and bool(torch.isfinite(only).all())
    assert rel < BOUND  # (the dead adapters' backward takes other GEMM routes: bf16-operand agreement, not bits)


# ------------------------------------------------------------------------------------------------ 6. the loops' helper
@pytest.mark.parametrize("T,Pn", [(2, 5), (0, 1)])
def test_answer_logits_reads_the_mask_rows_behind_the_prompt(T, Pn):
    from frozenbilm_amd import videoqa as P_vqa
    from tests.downstream_fixtures import Args, StubTokenizer

    Lt = 9
    cfg = _cfg(T, n_ans=24)
    A = build(cfg, _params(cfg, 89), Pn)
    tok, args = StubTokenizer(cfg.vocab_size), Args(max_feats=T, use_video=bool(T))
    batch = feed(cfg, T, Lt, seed=29, labels=False)
    ids = batch["input_ids"]
    ids[ids == tok.mask_token_id] = 7
    for b, c in enumerate((1, 4, 2)):  # one [MASK] per sample, inside the valid text
        ids[b, c] = tok.mask_token_id
    fd = _dev(batch)
    S = T + Pn + Lt
    with torch.no_grad():  # the rows route
        by_rows = P_vqa.answer_logits(A, tok, ids, args, **fd)
        full = A(**fd).logits
    by_full = P_vqa.answer_logits(A, tok, ids, args, **fd)  # grad mode without an opt-in: full logits, then the selection
    assert by_rows.shape == by_full.shape == (B, cfg.n_ans) and by_full.requires_grad
    want = full.reshape(B * S, -1)[torch.tensor([b * S + T + Pn + c for b, c in enumerate((1, 4, 2))], device=DEV)]
    d = (by_rows - by_full.detach()).abs().max().item()
    print(f"[answer_logits T={T} P={Pn}] rows route vs full-logits route: max-abs diff {d:.3g}")
    assert d < 2e-3 and (by_full.detach() - want).abs().max().item() < 2e-3
    unshifted = P_vqa.mask_row_logits(full, ids, tok, args)  # what the helper read before it knew the prompt
    assert (unshifted - by_rows).abs().max().item() > 1e-2 and (unshifted - by_full.detach()).abs().max().item() > 1e-2
