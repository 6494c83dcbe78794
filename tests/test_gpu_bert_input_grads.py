"""GPU: autograd through the BERT model's `video` and hidden states (bert_engine) against autograd of oracle/bert_oracle.py,
at the tiny BERT configuration of tests/test_gpu_bert.py.

Bounds: video.grad is held to the 2 % relative Frobenius norm every input gradient of the project is held to (dvideo is one more
bf16 GEMM on the rows that feed linear_video.weight.grad).  oracle/bert_oracle.py is plain fp32 (it has no bf16-operand mode), so
the trainable gradients next to it keep the bound the BERT suite holds them to against it, 6 % (tests/test_gpu_bert.py::_check_grads).  Unlike DeBERTa, BERT does not multiply its embeddings by the
mask, so a masked video slot has a gradient wherever something reads its row (a hidden-state term does)."""
import pytest
import torch

from frozenbilm_amd.model import BertConfig, BertForMaskedLM
from oracle import bert_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128,
             max_position_embeddings=64)
LIM = 6e-2
LIM_IN = 2e-2


def _ocfg():
    return O.BertOracleConfig(**SMALL, features_dim=32, max_feats=4)


def _model(P, train=False):
    m = BertForMaskedLM(BertConfig(**SMALL, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), features_dim=32, max_feats=4)
    m.load_state_dict(P, strict=False)
    m.to(DEV)
    return m.train(train)


def _batch(seed=5, B=3, T=4, Lt=12, V=300):
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, T, 32, generator=g)
    vm = torch.ones(B, T, dtype=torch.long)
    vm[1, 2:] = 0
    vm[2, 1] = 0  # (a zero inside the video slots)
    ids = torch.randint(5, V, (B, Lt), generator=g)
    am = torch.ones(B, Lt, dtype=torch.long)
    am[0, 9:] = 0
    am[2, 5:] = 0
    ids[am == 0] = 0
    labels = torch.full((B, Lt), -100)
    labels[:, 1::3] = ids[:, 1::3]
    labels[am == 0] = -100
    return dict(video=video, video_mask=vm, input_ids=ids, attention_mask=am, labels=labels)


def _to(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _trainable(P):
    for k, v in P.items():
        v.grad = None
        v.requires_grad_("linear_video" in k or (k.startswith("bert.") and "LayerNorm" in k))


def _rel(a, b):
    return (a.float().cpu() - b).norm().item() / (b.norm().item() + 1e-12)


def _worst(m, P):
    return sorted(((round(_rel(p.grad, P[n].grad), 5), n) for n, p in m.named_parameters() if p.requires_grad), reverse=True)


def _oracle_hidden(cfg, P, b, video):
    """every hidden state of the oracle: its own stages, composed as oracle.forward composes them"""
    mask = torch.cat([b["video_mask"], b["attention_mask"]], 1)
    ext = O.extended_mask(mask)
    x = O.embeddings(cfg, P, b["input_ids"], video)
    hs = [x]
    for i in range(cfg.num_hidden_layers):
        x = O.layer(cfg, P, i, x, ext)
        hs.append(x)
    return hs


def test_video_grad_vs_oracle():
    cfg = _ocfg()
    P = O.synth_params(cfg, seed=1, std=0.08, ln_jitter=0.1)
    b = _batch()
    _trainable(P)
    vc = b["video"].clone().requires_grad_()
    ref = O.forward(cfg, P, **{**b, "video": vc})
    ref["loss"].backward()
    m = _model(P)
    db = _to(b)
    v = db.pop("video").requires_grad_()
    out = m(**db, video=v)
    out.loss.backward()
    assert v.grad is not None and v.grad.shape == v.shape and v.grad.dtype == v.dtype
    rv, worst = _rel(v.grad, vc.grad), _worst(m, P)
    print(f"bert video.grad rel Frobenius {rv:.5f}; worst trainable {worst[:3]}")
    assert vc.grad.norm().item() > 0
    assert rv < LIM_IN, rv
    assert worst[0][0] < LIM, worst
    # a video that takes no gradient gets none; the half-precision caller gets its dtype back
    plain = b["video"].to(DEV)
    m(**db, video=plain).loss.backward()
    assert plain.grad is None
    vh = b["video"].to(DEV).half().requires_grad_()
    m(**db, video=vh).loss.backward()
    assert vh.grad.dtype == torch.float16 and vh.grad.shape == vh.shape


@pytest.mark.parametrize("with_loss", [True, False], ids=["loss+hidden", "hidden-only"])
def test_hidden_state_scalar_vs_oracle(with_loss):
    """scalar = [MLM loss +] sum_i <W_i, hs[i]> over every hidden state: trainable gradients and video.grad against oracle
    autograd of the same scalar"""
    cfg = _ocfg()
    nL = cfg.num_hidden_layers
    P = O.synth_params(cfg, seed=2, std=0.08, ln_jitter=0.1)
    b = _batch(seed=6)
    if not with_loss:
        b.pop("labels")
    B, S = 3, 16
    g = torch.Generator().manual_seed(3)
    W = [torch.randn(B, S, cfg.hidden_size, generator=g) / (B * S) for _ in range(nL + 1)]
    _trainable(P)
    vc = b["video"].clone().requires_grad_()
    hs_r = _oracle_hidden(cfg, P, b, vc)
    sr = sum((h * w).sum() for h, w in zip(hs_r, W))
    if with_loss:
        sr = sr + O.forward(cfg, P, **{**b, "video": vc})["loss"]
    sr.backward()
    m = _model(P)
    db = _to(b)
    v = db.pop("video").requires_grad_()
    out = m(**db, video=v, output_hidden_states=True)
    hs = out.hidden_states
    assert len(hs) == nL + 1 and all(h.requires_grad for h in hs)
    for h, r in zip(hs, hs_r):
        assert (h.detach().float().cpu() - r.detach()).abs().max().item() < 5e-2
    s = sum((h * w.to(DEV)).sum() for h, w in zip(hs, W))
    if with_loss:
        s = s + out.loss
    s.backward()
    rv, worst = _rel(v.grad, vc.grad), _worst(m, P)
    print(f"bert hidden-state scalar ({'with' if with_loss else 'without'} loss): video.grad {rv:.5f}; worst trainable {worst[:3]}")
    assert rv < LIM_IN, rv
    assert worst[0][0] < LIM, worst


def test_unused_hidden_states_change_nothing_and_train_mode_is_reproducible():
    cfg = _ocfg()
    P = O.synth_params(cfg, seed=4, std=0.08, ln_jitter=0.1)
    db = _to(_batch(seed=7))
    m = _model(P)
    m(**db).loss.backward()
    g0 = {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad}
    m.zero_grad(set_to_none=True)
    m(**db, output_hidden_states=True).loss.backward()
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, g0[n]), n
    # train mode: two identically seeded steps with a video gradient and a hidden-state term are bit-identical
    m.train()
    res = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        m.step_seed = 3
        v = db["video"].clone().requires_grad_()
        out = m(**{**db, "video": v}, output_hidden_states=True)
        (out.loss + out.hidden_states[1].square().mean()).backward()
        res.append((v.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad}))
    assert torch.equal(res[0][0], res[1][0]) and res[0][0].abs().max().item() > 0
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


def test_packed_rows_give_the_padded_grids_gradients():
    """model.packed_rows: video.grad and the gradients of a hidden-state scalar on the rows that exist equal those of the padded
    grid (1e-5, the bound of tests/test_gpu_bert_packed.py: the same arithmetic on fewer rows)"""
    cfg = _ocfg()
    P = O.synth_params(cfg, seed=5, std=0.08, ln_jitter=0.1)
    db = _to(_batch(seed=8))
    B, S = 3, 16
    W = torch.randn(B, S, cfg.hidden_size, generator=torch.Generator().manual_seed(9)).to(DEV) / (B * S)
    m = _model(P)
    res = {}
    for packed in (True, False):
        m.zero_grad(set_to_none=True)
        m.packed_rows = packed
        v = db["video"].clone().requires_grad_()
        out = m(**{**db, "video": v}, output_hidden_states=True)
        run = out._run
        assert (run.pk is not None) == packed
        if packed:
            have = torch.zeros(B * S, dtype=torch.bool, device=DEV)
            have[run.pk.sel] = True
            W = W * have.view(B, S, 1)
        (out.loss + sum((h * W).sum() for h in out.hidden_states)).backward()
        res[packed] = (v.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad})
    rv = (res[True][0] - res[False][0]).norm().item() / res[False][0].norm().item()
    worst = max((res[True][1][n] - res[False][1][n]).norm().item() / (res[False][1][n].norm().item() + 1e-12) for n in res[False][1])
    print(f"bert packed vs grid: video.grad {rv:.2e}, worst trainable {worst:.2e}")
    assert rv < 1e-5 and worst < 1e-5, (rv, worst)
