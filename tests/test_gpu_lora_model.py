"""GPU: LoRA on the frozen Q/K/V projections through the whole model -- W' = W + s.B.A merged into the packed operands once per
step, the two low-rank weight-gradient products per site and execution (token path and, for query / key, position path).

The tiny configuration of test_gpu_model.py with 2 layers (layer 0, then both enhanced-mask-decoder passes on layer 1), video
slots, S = 24: the position terms carry a large share of the scores.  The reference is the oracle on P' (W + s.B@A in place of
W: tests/test_lora_host.py pins that this IS the explicit low-rank form); bounds are those of the existing tests of the same
comparisons: logits 5e-2 max-abs / loss 2e-2 against the oracle (test_gpu_model.py), 2 % relative Frobenius per gradient
tensor against the bf16-operand oracle with replayed dropout masks and the GPU run's ReLU gates -- the judge of
test_train_mode_parity_with_replayed_dropout_masks for adapter.down / adapter.up --, rows route against full route 2e-3 / 1e-4
and packed against padded 2e-2 / 3e-2 (test_gpu_finetune_rows.py).

Measured on MI355X (worst relative Frobenius error of a lora_A / lora_B gradient against the oracle): see DESIGN.md "LoRA"."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import deberta_oracle as O  # noqa: E402
from tests.golden.make_goldens import _tiny_cfg, synth_batch  # noqa: E402
from tests.lora_refs import lora_names, lora_tensors, merged_params  # noqa: E402

DEV = "cuda"
QV, QKV, K = ("query_proj", "value_proj"), ("query_proj", "key_proj", "value_proj"), ("key_proj",)
RANK, ALPHA = 4, 8  # s = 2


def _cfg():
    return _tiny_cfg(num_hidden_layers=2)


def build(cfg, P, lora=None, rank=0, alpha=None, targets=QV, train=False):
    from frozenbilm_amd.model.config import DebertaV2Config
    from frozenbilm_amd.model.deberta import DebertaV2ForMaskedLM

    c = DebertaV2Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        max_position_embeddings=cfg.max_position_embeddings, position_buckets=cfg.position_buckets,
                        layer_norm_eps=cfg.layer_norm_eps, conv_kernel_size=cfg.conv_kernel_size)
    m = DebertaV2ForMaskedLM(c, max_feats=cfg.max_feats, features_dim=cfg.features_dim, ds_factor_attn=cfg.ds_factor_attn,
                             ds_factor_ff=cfg.ds_factor_ff, lora_rank=rank, lora_alpha=alpha, lora_targets=targets)
    missing, unexpected = m.load_state_dict({**P, **(lora or {})}, strict=False)
    assert not unexpected, unexpected
    assert all("position_ids" in k or (lora is None and ".lora_" in k) for k in missing), missing
    m.to(DEV)
    m.train(train)
    return m


def to_dev(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def _rel_fro(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


def _grads(m):
    return {n: (p.grad.detach().float().cpu().clone() if p.grad is not None else None) for n, p in m.named_parameters() if p.requires_grad}


def _gates_of(run, cfg):
    g = []
    for sv in run.layers:
        g += [(sv.z1[:, : cfg.hidden_size // cfg.ds_factor_attn] > 0).cpu(), (sv.z2[:, : cfg.hidden_size // cfg.ds_factor_ff] > 0).cpu()]
    return g


@pytest.fixture(scope="module")
def base():
    """parameters, batch and the rank-0 model's results (eval forward; train step at torch seed 777), computed once"""
    cfg = _cfg()
    P = O.synth_params(cfg, seed=51, std=0.05, ln_jitter=0.1)
    batch = synth_batch(cfg, B=3, L=14, seed=11)
    m = build(cfg, P)
    with torch.no_grad():
        ev = m(**to_dev(batch))
        ev = (ev.loss.clone(), ev.logits.clone())
    torch.manual_seed(777)
    m = build(cfg, P, train=True)
    out = m(**to_dev(batch))
    out.loss.backward()
    tr = (out.loss.detach().clone(), out.logits.detach().clone(), _grads(m))
    return dict(cfg=cfg, P=P, batch=batch, eval=ev, train=tr)


# ------------------------------------------------------------------------------------------------ B = 0
@pytest.mark.parametrize("targets", [QV, QKV], ids=["qv", "qkv"])
def test_zero_B_is_the_rank0_model(base, targets):
    cfg, P, batch = base["cfg"], base["P"], base["batch"]
    lora = lora_tensors(cfg.hidden_size, 2, RANK, targets, seed=3, zero_B=True)
    m = build(cfg, P, lora, RANK, ALPHA, targets)
    with torch.no_grad():
        out = m(**to_dev(batch))
    assert torch.equal(out.loss, base["eval"][0]) and torch.equal(out.logits, base["eval"][1])
    torch.manual_seed(777)
    m = build(cfg, P, lora, RANK, ALPHA, targets, train=True)
    out = m(**to_dev(batch))
    out.loss.backward()
    loss0, logits0, g0 = base["train"]
    assert torch.equal(out.loss.detach(), loss0) and torch.equal(out.logits.detach(), logits0)
    g = _grads(m)
    fallback = []
    for n, ref in g0.items():
        if not torch.equal(g[n], ref):  # the fallback test_gpu_partial_finetune.py names: the project's 2 % relative Frobenius
            fallback.append((n, _rel_fro(g[n], ref)))
            assert fallback[-1][1] < 2e-2, fallback[-1]
    print(f"[B = 0, {targets}] pre-existing gradients that are not the rank-0 model's bit for bit: {fallback or 'none'}")
    for nm in lora_names(2, targets):
        assert torch.count_nonzero(g[nm + ".lora_A.weight"]) == 0, nm   # dA = s.(dY.B)^T.X with B = 0: exactly zero
        assert g[nm + ".lora_B.weight"].abs().max().item() > 0, nm


# ------------------------------------------------------------------------------------------------ random A, B against the oracle
@pytest.mark.parametrize("targets", [QV, QKV, K], ids=["qv", "qkv", "k"])
def test_random_lora_against_the_oracle(base, targets):
    from tests.dropout_replay import ReplayedMasks

    cfg, P, batch = base["cfg"], base["P"], base["batch"]
    B = batch["input_ids"].shape[0]
    s = ALPHA / RANK
    lora = lora_tensors(cfg.hidden_size, 2, RANK, targets, seed=5, sigma=0.02)
    # ---- eval logits against the oracle on P'
    m = build(cfg, P, lora, RANK, ALPHA, targets)
    with torch.no_grad():
        out = m(**to_dev(batch))
        ref = O.forward(merged_params(P, lora, s)[0], cfg, **batch)
    d_log = (out.logits.float().cpu() - ref["logits"]).abs().max().item()
    d_base = (out.logits - base["eval"][1]).abs().max().item()
    print(f"[{targets}] eval logits max-abs diff to the oracle on P' {d_log:.3e} (to the rank-0 model: {d_base:.3e})")
    assert d_log < 5e-2 and abs(out.loss.item() - ref["loss"].item()) < 2e-2
    assert d_base > 1e-3, "the low-rank update made no difference: the comparison would prove nothing"
    # ---- train mode, replayed dropout: every gradient against oracle autograd in bf16_operands mode
    torch.manual_seed(777)
    m = build(cfg, P, lora, RANK, ALPHA, targets, train=True)
    out = m(**to_dev(batch))
    run = out.__dict__["_run"]
    c = m.config
    masks = ReplayedMasks(run, cfg, cfg.num_attention_heads, c.hidden_dropout_prob, c.attention_probs_dropout_prob, m.adapter_dropout)
    gates = _gates_of(run, cfg)
    assert len(run.layers) == cfg.num_hidden_layers + 1 and masks.seed_emb != 0
    out.loss.backward()
    g = _grads(m)
    for k, v in P.items():
        v.requires_grad_(O.is_trainable(k))
        v.grad = None
    Pm, leaves = merged_params(P, lora, s, requires_grad=True)
    with O.bf16_operands(), O.adapter_gates([g_.view(B, -1, g_.shape[-1]) for g_ in gates]), O.dropout_masks(masks):
        ref = O.forward(Pm, cfg, **batch)
        ref["loss"].backward()
    assert masks.exhausted(), masks.asked
    want = {n: v.grad for n, v in P.items() if v.requires_grad}
    want.update({n: v.grad for n, v in leaves.items()})
    assert set(want) == set(g), set(want) ^ set(g)
    worst = sorted(((round(_rel_fro(g[n], want[n]), 4), n) for n in want), reverse=True)
    worst_lora = [w for w in worst if ".lora_" in w[1]]
    print(f"[{targets}] train-mode parity: loss {out.loss.item():.5f} vs {ref['loss'].item():.5f}, worst LoRA gradients "
          f"{worst_lora[:4]}, worst others {[w for w in worst if '.lora_' not in w[1]][:2]}")
    assert abs(out.loss.item() - ref["loss"].item()) < 2e-2
    assert (out.logits.float().cpu() - ref["logits"]).abs().max().item() < 5e-2
    assert all(want[n].abs().max().item() > 0 for n in leaves)
    assert worst[0][0] < 2e-2, worst[:8]
    for v in P.values():
        v.requires_grad_(False)
        v.grad = None


# ------------------------------------------------------------------------------------------------ further cases
def _lora_model(base, targets=QKV, train=True, seed=5):
    cfg = base["cfg"]
    lora = lora_tensors(cfg.hidden_size, 2, RANK, targets, seed=seed, sigma=0.02)
    torch.manual_seed(777)
    return build(cfg, base["P"], lora, RANK, ALPHA, targets, train=train), lora


def _step(m, batch):
    m.zero_grad(set_to_none=True)
    m.step_seed = 0
    out = m(**to_dev(batch))
    out.loss.backward()
    return out.loss.detach().clone(), out.logits.detach().clone(), _grads(m)


def test_two_identical_steps_are_bit_identical(base):
    m, _ = _lora_model(base)
    a, b = _step(m, base["batch"]), _step(m, base["batch"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_optimizer_step_moves_the_next_forward_to_the_oracles(base):
    from frozenbilm_amd.optim import FusedAdam

    cfg, P, batch = base["cfg"], base["P"], base["batch"]
    m, _ = _lora_model(base, train=False)
    opt = FusedAdam(m, lr=1e-2)
    with torch.no_grad():
        before = m(**to_dev(batch)).logits.clone()
    out = m(**to_dev(batch))
    out.loss.backward()
    opt.step()
    with torch.no_grad():
        after = m(**to_dev(batch)).logits.float().cpu()
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items() if "position_ids" not in k}
    lora = {k: v for k, v in sd.items() if ".lora_" in k}
    Pn = {k: sd[k] for k in P}
    with torch.no_grad():
        ref = O.forward(merged_params(Pn, lora, ALPHA / RANK)[0], cfg, **batch)["logits"]
    moved = (after - before.float().cpu()).abs().max().item()
    d = (after - ref).abs().max().item()
    print(f"one Adam step (lr 1e-2): logits moved by {moved:.3e}, differ from the oracle with the updated parameters by {d:.3e}")
    assert moved > 5e-2, "the step did not move the logits beyond the comparison's bound"
    assert d < 5e-2
    assert all(torch.count_nonzero(v) > 0 for v in lora.values())


def test_inside_weights_frozen_two_forwards_compose_once(base):
    m, _ = _lora_model(base, train=False)
    feed = to_dev(base["batch"])
    with torch.no_grad():
        first = m(**feed).logits.clone()
        n0 = m.engine().lora_composes
        m(**feed)
        assert m.engine().lora_composes == n0 + 1  # outside: every forward rebuilds the operands
        with m.weights_frozen():
            a = m(**feed).logits.clone()
            n1 = m.engine().lora_composes
            b = m(**feed).logits.clone()
            assert m.engine().lora_composes == n1 <= n0 + 2
    assert torch.equal(a, b) and torch.equal(a, first)


def test_merge_lora_keeps_the_logits_and_exports_a_plain_checkpoint(base):
    cfg, batch = base["cfg"], base["batch"]
    m, lora = _lora_model(base, train=False)
    feed = to_dev(batch)
    with torch.no_grad():
        before = m(**feed)
        before = (before.loss.clone(), before.logits.clone())
    w0 = {nm: m.get_param(nm + ".weight").detach().clone() for nm in m.lora_names()}
    m.merge_lora()
    with torch.no_grad():
        after = m(**feed)
    assert torch.equal(after.loss, before[0]) and torch.equal(after.logits, before[1])
    for nm in m.lora_names():
        assert torch.count_nonzero(m.get_param(nm + ".lora_B.weight")) == 0
        W = m.get_param(nm + ".weight").detach()
        want = w0[nm].double() + (ALPHA / RANK) * (lora[nm + ".lora_B.weight"].double() @ lora[nm + ".lora_A.weight"].double()).to(DEV)
        assert not torch.equal(W, w0[nm]) and (W.double() - want).abs().max().item() < 1e-6
    # the state_dict without its lora_* keys is a plain checkpoint: a rank-0 model loaded from it gives the same logits
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items() if ".lora_" not in k}
    plain = build(cfg, {k: v for k, v in sd.items() if "position_ids" not in k})
    assert set(plain.state_dict()) == set(sd)
    with torch.no_grad():
        out = plain(**feed)
    assert torch.equal(out.logits, before[1])


def test_frozen_lora_B_of_layer_0(base):
    from frozenbilm_amd.optim import FusedAdam

    batch = base["batch"]
    m, _ = _lora_model(base)
    full = _step(m, batch)
    name = "deberta.encoder.layer.0.attention.self.query_proj.lora_B.weight"
    p = m.get_param(name)
    p.requires_grad_(False)
    bits = p.detach().clone()
    opt = FusedAdam(m, lr=1e-2)
    loss, logits, g = _step(m, batch)
    assert p.grad is None and name not in g
    assert torch.equal(loss, full[0]) and torch.equal(logits, full[1])
    for n, ref in full[2].items():
        if n != name:
            assert torch.equal(g[n], ref), n
    a_name = name.replace("lora_B", "lora_A")
    a_bits = m.get_param(a_name).detach().clone()
    opt.step()
    assert torch.equal(p.detach(), bits), "a frozen lora_B moved"
    assert not torch.equal(m.get_param(a_name).detach(), a_bits)
    # its value still enters the compose: zeroing it (through .data, outside weights_frozen) changes the logits
    m.eval()
    with torch.no_grad():
        l1 = m(**to_dev(batch)).logits.clone()
        p.data.zero_()
        l2 = m(**to_dev(batch)).logits
    assert not torch.equal(l1, l2)


def test_rows_route_and_packed_rows_against_the_full_route(base):
    cfg, batch = base["cfg"], dict(base["batch"])
    batch.pop("labels")
    m, _ = _lora_model(base, train=False)
    feed = to_dev(batch)
    Bn, Lt = batch["input_ids"].shape
    S = cfg.max_feats + Lt
    rows = (torch.arange(Bn) * S + cfg.max_feats + batch["attention_mask"].sum(1) // 2).to(DEV)
    tgt = torch.randint(0, cfg.vocab_size, (Bn,), generator=torch.Generator().manual_seed(1)).to(DEV)
    res = {}
    for kind in ("full", "rows", "packed"):
        m.zero_grad(set_to_none=True)
        m.packed_rows = kind == "packed"
        if kind == "full":
            out = m(**feed)
            logits = out.logits.reshape(Bn * S, -1)[rows]
        else:
            out = m(**feed, logit_rows=rows)
            logits = out.logits
            assert (out._run.pk is not None) == (kind == "packed")
        torch.nn.functional.cross_entropy(logits, tgt).backward()
        res[kind] = (logits.detach().clone(), _grads(m))
    m.packed_rows = False
    for kind, ref, tol_l, tol_g in (("rows", "full", 2e-3, 1e-4), ("packed", "rows", 2e-2, 3e-2)):
        d_log = (res[kind][0] - res[ref][0]).abs().max().item()
        worst = max((_rel_fro(res[kind][1][n], res[ref][1][n]), n) for n in res[ref][1])
        print(f"[{kind} vs {ref}] logits max-abs diff {d_log:.3g}, worst gradient Frobenius diff {worst}")
        assert all(res[ref][1][n].norm().item() > 0 for n in res[ref][1])
        assert d_log < tol_l and worst[0] < tol_g, (kind, d_log, worst)


def test_decoder_rows_and_graph_switches_take_the_checked_routes(base):
    """decoder_rows, training_graphs and finetune_graphs are not served with LoRA: the calls go to the full / eager route and
    give its results bit for bit"""
    batch = base["batch"]
    m, _ = _lora_model(base)
    ref = _step(m, batch)
    m.decoder_rows = True
    got = _step(m, batch)
    m.decoder_rows = False
    m.training_graphs = m.finetune_graphs = m.inference_graphs = True
    got2 = _step(m, batch)
    assert not m.__dict__.get("_train_graphs")
    for g_ in (got, got2):
        assert torch.equal(g_[0], ref[0]) and torch.equal(g_[1], ref[1])
        for n in ref[2]:
            assert torch.equal(g_[2][n], ref[2][n]), n


# ------------------------------------------------------------------------------------------------ true widths
def test_gradients_at_true_widths_against_the_bf16_operand_oracle():
    """H = 1536, 24 heads, I = 6144, 192-wide adapters, 2 layers, B = 2, S = 74, r = 16 on (q, k, v): every gradient against the
    oracle with the HIP path's arithmetic contract and the ReLU gates the GPU run took (the judge of
    test_gradients_vs_bf16_operand_oracle_tight)."""
    cfg = O.OracleConfig()
    cfg.num_hidden_layers, cfg.vocab_size = 2, 4096
    P = O.synth_params(cfg, seed=41, std=0.02, ln_jitter=0.1)
    Bn, Lt, r, alpha = 2, 74 - cfg.max_feats, 16, 32
    batch = synth_batch(cfg, B=Bn, L=Lt, seed=7)
    lora = lora_tensors(cfg.hidden_size, 2, r, QKV, seed=9, sigma=0.02)
    m = build(cfg, P, lora, r, alpha, QKV)
    out = m(**to_dev(batch))
    assert out._run.S == 74
    gates = _gates_of(out.__dict__["_run"], cfg)
    out.loss.backward()
    g = _grads(m)
    for k, v in P.items():
        v.requires_grad_(O.is_trainable(k))
    Pm, leaves = merged_params(P, lora, alpha / r, requires_grad=True)
    with O.bf16_operands(), O.adapter_gates([g_.view(Bn, -1, g_.shape[-1]) for g_ in gates]):
        ref = O.forward(Pm, cfg, **batch)
        ref["loss"].backward()
    want = {n: v.grad for n, v in P.items() if v.requires_grad}
    want.update({n: v.grad for n, v in leaves.items()})
    assert set(want) == set(g)
    worst = sorted(((round(_rel_fro(g[n], want[n]), 4), n) for n in want), reverse=True)
    print("true widths, r = 16: worst LoRA gradients", [w for w in worst if ".lora_" in w[1]][:4], "worst others",
          [w for w in worst if ".lora_" not in w[1]][:2])
    assert abs(out.loss.item() - ref["loss"].item()) < 5e-3
    assert worst[0][0] < 2e-2, worst[:8]
