"""Training with relative-position maps other than FrozenBiLM's (256 buckets / 512 positions) on a real MI355X.

Coarse log-bucket maps (64 / 512, 128 / 512, 32 / 128) put up to a few dozen relative positions on one table row, and clamped
tables (position_buckets <= 0) put every delta beyond the span on the two edge rows -- hundreds of them at S = 512.  The
position-table gradients of such maps run the prefix-difference kernel of fbl_attn_pos_grad; the recompute route's shear
pass stores plainly only where a clamped map is injective (|delta| < att_span - 1).  Checked at three levels: the kernel against
an fp32 index_add reference, the attention backward stage on both routes against autograd, and one training step of a tiny
model against the CPU oracle (plus a graph replay against the eager step).
"""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import deberta_oracle as O  # noqa: E402
from tests.golden.make_goldens import _tiny_cfg, synth_batch  # noqa: E402
from tests.gpu_refs import bf, heads, ref_attention, stats, unheads  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


def _map(pb, mr):
    return types.SimpleNamespace(position_buckets=pb, max_rel=mr, att_span=pb if pb > 0 else mr)


def _relidx(S, cfg):
    from frozenbilm_amd.model.relpos import rel_index_vector

    return torch.from_numpy(rel_index_vector(S, cfg.position_buckets, cfg.max_rel, cfg.att_span).astype(np.int16)).to(DEV)


def close(got, ref, rtol, atol, name=""):
    assert torch.allclose(got.float(), ref.float(), rtol=rtol, atol=atol), stats(name, got.float(), ref.float())


# ------------------------------------------------------------------------------------------------ kernel
MAPS = [(64, 512, 266), (64, 512, 512), (128, 512, 512), (32, 128, 128), (0, 128, 300), (0, 128, 512)]


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("pb,mr,S", MAPS, ids=[f"{a}_{b}_S{c}" for a, b, c in MAPS])
def test_pos_grad_kernel_any_bucket_map(L, pb, mr, S, B, E):
    """fbl_attn_pos_grad on maps with more than 8 deltas per table row, both directions: neg = 0 (dPK from dS and q) and
    neg = 1 (dPQ from dS^T and k) against index_add over the index map in fp32 from the same bf16 inputs.  B = 4: ragged klen;
    with E = 3 also packed rows (row0).  X is NaN outside the [kl64 x kl64] corner the attention kernels write (zeros between
    klen and kl64), so a read beyond it shows.  Two calls give bit-identical outputs."""
    from frozenbilm_amd.attn_bwd import _delta_ranges, _relidx_range

    cfg = _map(pb, mr)
    nh, H = 2, 128
    Sp = (S + 63) // 64 * 64
    dlo, dcnt, cmax = _delta_ranges(S, cfg, torch.device(DEV), limit=None)
    assert cmax > 8  # the maps this file is about
    rmin, rcnt = _relidx_range(S, cfg)
    kl = [S] if B == 1 else [S, max(1, S // 3), S - 37, 45]
    klen = torch.tensor(kl, dtype=torch.int32, device=DEV) if B > 1 else None
    packed = B > 1 and E == 3
    row0 = torch.tensor([0] + list(np.cumsum(kl)), dtype=torch.int32, device=DEV) if packed else None
    nrows = sum(kl) if packed else B * S
    g = torch.Generator(device="cpu").manual_seed(100 * pb + S + 7 * B + E)
    R = _relidx(S, cfg).long() - rmin
    ii = torch.arange(S, device=DEV)
    Rq = R[ii[:, None] - ii[None, :] + S - 1]  # [i, j] -> table row - rmin
    for neg in (0, 1):
        Xs, Ys, ref = [], [], torch.zeros(E, nh, rcnt, 64, device=DEV)
        for e in range(E):
            X = torch.full((B, nh, Sp, Sp), float("nan"), dtype=BF16)
            Xv = torch.randn(B, nh, S, S, generator=g).to(BF16)
            Yt = torch.randn(nrows, 3 * H, generator=g).to(BF16).to(DEV)
            Y = Yt[:, (1 - neg) * H:(2 - neg) * H]  # q or k: a column block of a wider buffer, ldy = 3H
            for b in range(B):
                k64 = (kl[b] + 63) // 64 * 64
                X[b, :, :k64, :k64] = 0
                X[b, :, :kl[b], :kl[b]] = Xv[b, :, :kl[b], :kl[b]]
            X = X.to(DEV)
            Xs.append(X)
            Ys.append(Y)
            for b in range(B):
                n = kl[b]
                r0 = int(row0[b]) if packed else b * S
                Yb = Y[r0:r0 + n].float().view(n, nh, 64).permute(1, 0, 2)  # [nh, k, 64]
                Xb = X[b, :, :n, :n].float()  # [nh, k, col]
                # neg = 0: row k = query i, column j, table row idx(i - j); neg = 1: row k = key j, column i, idx(i - j)
                Rk = Rq[:n, :n] if neg == 0 else Rq[:n, :n].t()
                G = torch.zeros(nh, n, rcnt, device=DEV).scatter_add_(2, Rk.expand(nh, n, n), Xb)  # [nh, k, r]
                ref[e] += torch.einsum("hkr,hkd->hrd", G.to(BF16).float(), Yb)  # G meets the matrix cores as bf16
        outs = []
        for _ in range(2):
            out = torch.full((E, nh, rcnt, 64), float("nan"), device=DEV)
            L.attn_pos_grad(neg, Xs, Ys, dlo, dcnt, cmax, out, B, S, Sp, nh, rcnt, klen=klen, row0=row0)
            outs.append(out)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), "not bit-reproducible"
        sc = ref.abs().max().item()
        close(outs[0], ref, 1e-2, 2e-3 * sc, f"neg={neg}")


# ------------------------------------------------------------------------------------------------ attention backward stage
STAGE = [(64, 512, 2, 266), (128, 512, 1, 512), (0, 128, 2, 300), (0, 128, 1, 512)]


@pytest.mark.parametrize("saved_p", [False, True], ids=["recompute", "saved_p"])
@pytest.mark.parametrize("pb,mr,B,S", STAGE, ids=[f"{a}_{b}_S{d}" for a, b, c, d in STAGE])
def test_attention_bwd_any_bucket_map(L, pb, mr, B, S, saved_p):
    """disent_attn_bwd on both routes against autograd of the reference attention, with eng.cfg / relidx set to the map (the
    stand-ins and bounds of test_gpu_kernels.py::test_attention_bwd).  The clamped maps at S > max_relative_positions run the
    recompute route's shear pass with plain stores only inside the span, atomics on the two edge rows."""
    from frozenbilm_amd.attn_bwd import disent_attn_bwd

    cfg = _map(pb, mr)
    nh, H = 2, 128
    span2 = 2 * cfg.att_span
    relidx = _relidx(S, cfg)
    g = torch.Generator(device="cpu").manual_seed(S + pb)
    qkv = bf(torch.randn(B * S, 3 * H, generator=g) * 0.5).to(BF16).to(DEV)
    pqk = bf(torch.randn(span2, 2 * H, generator=g) * 0.5).to(BF16).to(DEV)
    mask = torch.ones(B, S, dtype=torch.int32, device=DEV)
    mask[0, S - 5:] = 0
    if B > 1:
        mask[1, S // 2:] = 0
    klen = (mask * torch.arange(1, S + 1, device=DEV, dtype=torch.int32)).amax(1).to(torch.int32).contiguous()
    lin_f = min(pb // 2, cfg.att_span) if pb > 0 else 0  # the forward's affine addressing (engine.lin_span)
    Sp = (S + 63) // 64 * 64
    ctx = torch.zeros(B * S, H, dtype=BF16, device=DEV)
    lse = torch.empty(B, nh, S, device=DEV)
    ps = ms = None
    if saved_p:
        ps = torch.full((B, nh, Sp, Sp), float("nan"), dtype=BF16, device=DEV)
        ms = torch.full((B, nh, Sp // 64, S), float("nan"), dtype=F32, device=DEV)
    scale = 1 / math.sqrt(192)
    L.disent_attn_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], pqk[:, H:], pqk[:, :H], relidx, mask.view(-1), scale, ctx, lse,
                      B, S, Sp, nh, span2, klen=klen, lin=lin_f, psave=ps, msave=ms)
    dctx = bf(torch.randn(B * S, H, generator=g)).to(BF16).to(DEV)
    qkvf = qkv.float().requires_grad_(True)
    pqkf = pqk.float().requires_grad_(True)
    q, k, v = (heads(qkvf[:, i * H:(i + 1) * H], B, S, nh) for i in range(3))
    pq = pqkf[:, :H].view(-1, nh, 64).permute(1, 0, 2)
    pk = pqkf[:, H:].view(-1, nh, 64).permute(1, 0, 2)
    ref, _ = ref_attention(q, k, v, pk, pq, relidx, mask, scale)
    (unheads(ref) * dctx.float()).sum().backward()

    class E:  # minimal engine/run/sv stand-ins
        pass

    eng, run, sv = E(), E(), E()
    eng.H, eng.nh, eng.span2, eng.dev = H, nh, span2, torch.device(DEV)
    eng.relidx = lambda S_: relidx
    eng.cfg = cfg
    run.B, run.S, run.mask_i32, run.p_att = B, S, mask.view(-1), 0.0
    run.klen, run.border = klen, None
    sv.qkv, sv.pqk, sv.ctx, sv.lse, sv.seed_att = qkv, pqk, ctx, lse, 0
    if saved_p:
        sv.psave, sv.msave = ps, ms
    dqkv = torch.zeros(B * S, 3 * H, dtype=BF16, device=DEV)
    dpqk = torch.zeros(span2, 2 * H, dtype=BF16, device=DEV)
    disent_attn_bwd(eng, run, sv, dctx, dqkv, dpqk)
    gq = qkvf.grad
    sc = gq.abs().max().item()
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)), ("dV", slice(2 * H, 3 * H))):
        close(dqkv[:, sl], gq[:, sl], 3e-2, 2e-2 * sc, name)
    sp = pqkf.grad.abs().max().item()
    close(dpqk[:, H:], pqkf.grad[:, H:], 3e-2, 2e-2 * sp, "dPK")
    close(dpqk[:, :H], pqkf.grad[:, :H], 3e-2, 2e-2 * sp, "dPQ")


# ------------------------------------------------------------------------------------------------ model
def _build(cfg, P, max_rel, train=False, engine_options=None):
    from frozenbilm_amd.model.config import DebertaV2Config
    from frozenbilm_amd.model.deberta import DebertaV2ForMaskedLM

    c = DebertaV2Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                        num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                        max_position_embeddings=cfg.max_position_embeddings, position_buckets=cfg.position_buckets,
                        max_relative_positions=max_rel, layer_norm_eps=cfg.layer_norm_eps,
                        conv_kernel_size=cfg.conv_kernel_size)
    m = DebertaV2ForMaskedLM(c, max_feats=cfg.max_feats, features_dim=cfg.features_dim, ds_factor_attn=cfg.ds_factor_attn,
                             ds_factor_ff=cfg.ds_factor_ff, n_ans=cfg.n_ans)
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected, unexpected
    assert all("position_ids" in k for k in missing), missing
    if engine_options:
        m.engine_options = dict(engine_options)
    m.to(DEV)
    m.train(train)
    return m


MODEL_MAPS = [(64, -1), (0, 128)]


@pytest.mark.parametrize("attn_save_p", [True, False], ids=["saved_p", "recompute"])
@pytest.mark.parametrize("pb,mr", MODEL_MAPS, ids=["buckets64", "clamped128"])
def test_training_step_vs_oracle_any_bucket_map(pb, mr, attn_save_p):
    """One backward of a tiny DeBERTa (S = 10 video + 256 text = 266) with a coarse bucket map and with a clamped table, against
    the CPU oracle: loss within 2e-2, every trainable gradient within the bounds of
    test_gpu_model.py::test_backward_vs_oracle_larger_batch."""
    cfg = _tiny_cfg(position_buckets=pb, max_relative_positions=mr)
    P = O.synth_params(cfg, seed=43, std=0.05, ln_jitter=0.1)
    m = _build(cfg, P, mr, engine_options={"attn_save_p": attn_save_p})
    batch = synth_batch(cfg, B=4, L=256, seed=9)
    for k, v in P.items():
        v.requires_grad_(O.is_trainable(k))
    ref = O.forward(P, cfg, **batch)
    ref["loss"].backward()
    out = m(**{k: v.to(DEV) for k, v in batch.items()})
    out.loss.backward()
    assert abs(out.loss.item() - ref["loss"].item()) < 2e-2
    worst = []
    for name, p in m.named_parameters():
        if p.requires_grad:
            r = P[name].grad
            assert p.grad is not None and r is not None, name
            fro = (p.grad.float().cpu() - r).norm().item() / max(r.norm().item(), 1e-9)
            worst.append((round(fro, 4), name))
    worst.sort(reverse=True)
    print("worst relative Frobenius grad errors:", worst[:8])
    assert any(n == "deberta.encoder.LayerNorm.weight" for _, n in worst)  # the position table's LayerNorm: fed by pos_grad
    strict = [w for w in worst if "adapter.down" not in w[1]]
    assert strict[0][0] < 4e-2, strict[:6]
    assert worst[0][0] < 0.18, worst[:6]


def test_graphed_training_step_equals_the_eager_step_coarse_map():
    """model.training_graphs with a 64-bucket map: three optimizer steps of one shape (warm-up + capture, then replays) leave
    exactly the parameters and losses of the eager loop."""
    from frozenbilm_amd.optim import FusedAdam

    cfg = _tiny_cfg(position_buckets=64)
    P = O.synth_params(cfg, seed=48, std=0.05, ln_jitter=0.1)
    batches = [{k: v.to(DEV) for k, v in synth_batch(cfg, B=2, L=256, seed=80 + i).items()} for i in range(3)]
    results = []
    for graphs in (False, True):
        torch.manual_seed(321)
        m = _build(cfg, P, -1, train=True)
        m.training_graphs = graphs
        opt = FusedAdam(m, lr=1e-3, betas=(0.9, 0.95))
        losses = []
        for b in batches:
            opt.zero_grad(set_to_none=False)
            out = m(**b)
            out.loss.backward()
            opt.step(clip_max_norm=1.0)
            losses.append(out.loss.item())
        results.append((losses, {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}))
        if graphs:
            assert len(m.__dict__.get("_train_graphs", {})) == 1
    (l0, p0), (l1, p1) = results
    assert l0 == l1, (l0, l1)
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
