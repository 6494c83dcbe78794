"""GPU: the BERT variant's fused attention (include/fbl_mha.h) against fp32 torch of the reference formula
softmax(Q.K^T/8 + (1 - mask) * -10000) . V  (oracle/bert_oracle.py self_attention, model/bert.py:138-191)."""
import math

import pytest
import torch

from tests.dropout_replay import attn_mask
from tests.gpu_refs import bf, heads, stats, unheads

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SCALE = 1 / math.sqrt(64)


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


def close(got, ref, rtol, atol, name=""):
    assert torch.allclose(got.float(), ref.float(), rtol=rtol, atol=atol), stats(name, got.float(), ref.float())


def _inputs(B, S, nh, seed, scale=1.0):
    """q|k|v in one bf16 [B*S, 3H] buffer (row stride 3H, as the engine's fused QKV GEMM leaves it) and a mask with ragged
    right padding, zeros inside the leading (video) slots and -- sample 2 -- no valid key at all"""
    H = nh * 64
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * S, 3 * H, generator=g) * scale).to(BF16).to(DEV)
    mask = torch.ones(B, S, dtype=torch.int32)
    if B > 1:
        mask[1, max(1, (2 * S) // 3):] = 0
        mask[1, 1:min(S, 4)] = 0
    if B > 2:
        mask[2] = 0
    if B > 3:
        mask[3, max(1, S // 5):] = 0
    return qkv, mask.to(DEV), H


def _klen(mask):
    S = mask.shape[1]
    return (mask * torch.arange(1, S + 1, device=mask.device, dtype=torch.int32)).amax(1).to(torch.int32).contiguous()


def _ref(qkv, mask, B, S, nh, keep=None):
    H = nh * 64
    q, k, v = (heads(qkv[:, i * H:(i + 1) * H], B, S, nh) for i in range(3))
    s = torch.einsum("bhid,bhjd->bhij", q, k) * SCALE + (1.0 - mask[:, None, None, :].float()) * -10000.0
    lse = torch.logsumexp(s, -1)
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep
    return torch.einsum("bhij,bhjd->bhid", p, v), lse


def _fwd(L, qkv, mask, B, S, nh, **kw):
    H = nh * 64
    ctx = torch.full((B * S, H), float("nan"), dtype=BF16, device=DEV)
    lse = torch.full((B, nh, S), float("nan"), device=DEV)
    L.mha_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], mask.view(-1), SCALE, ctx, lse, B, S, nh, **kw)
    return ctx, lse


def _bwd(L, qkv, mask, ctx, lse, dctx, B, S, nh, **kw):
    H = nh * 64
    Dv = torch.empty(B, nh, S, device=DEV)
    L.attn_rowdot(dctx, ctx, Dv, B, S, nh)
    dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=BF16, device=DEV)
    L.mha_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], dctx, mask.view(-1), lse, Dv, SCALE, dqkv[:, :H], dqkv[:, H:2 * H],
              dqkv[:, 2 * H:], B, S, nh, **kw)
    return dqkv


SHAPES = [(B, S, nh) for S in (1, 16, 37, 64, 74, 129, 266, 512) for nh in (12, 16) for B in ([3] if S == 512 else [4])]


@pytest.mark.parametrize("B,S,nh", SHAPES)
def test_mha_fwd(L, B, S, nh):
    qkv, mask, H = _inputs(B, S, nh, seed=S + nh)
    ctx, lse = _fwd(L, qkv, mask, B, S, nh)
    ref, rlse = _ref(qkv.float(), mask, B, S, nh)
    close(heads(ctx.float(), B, S, nh), ref, 2e-2, 2e-2, f"ctx S={S} nh={nh}")
    close(lse, rlse, 1e-3, 1e-3, "lse")  # every row, padded query rows and the sample without a valid key included
    # skipping the key tiles beyond the last valid key (klen) and the longest-first dispatch order change no bit
    kl = _klen(mask)
    c2, l2 = _fwd(L, qkv, mask, B, S, nh, klen=kl, border=torch.argsort(kl, descending=True, stable=True).to(torch.int32))
    assert torch.equal(ctx, c2) and torch.equal(lse, l2)


@pytest.mark.parametrize("B,S,nh", SHAPES)
def test_mha_bwd(L, B, S, nh):
    qkv, mask, H = _inputs(B, S, nh, seed=100 + S + nh, scale=0.7)
    kl = _klen(mask)
    ctx, lse = _fwd(L, qkv, mask, B, S, nh, klen=kl)
    g = torch.Generator().manual_seed(7)
    dctx = torch.randn(B * S, H, generator=g).to(BF16).to(DEV)
    qf = qkv.float().requires_grad_(True)
    ref, _ = _ref(qf, mask, B, S, nh)
    (unheads(ref) * dctx.float()).sum().backward()
    dqkv = _bwd(L, qkv, mask, ctx, lse, dctx, B, S, nh, klen=kl)
    sc = qf.grad.abs().max().item()
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)), ("dV", slice(2 * H, 3 * H))):
        close(dqkv[:, sl], qf.grad[:, sl], 3e-2, 2e-2 * sc, f"{name} S={S} nh={nh}")
    # no atomics: bit-identical run to run; the tiles beyond klen contribute exactly nothing
    assert torch.equal(dqkv, _bwd(L, qkv, mask, ctx, lse, dctx, B, S, nh, klen=kl))
    c0, l0 = _fwd(L, qkv, mask, B, S, nh)
    assert torch.equal(dqkv, _bwd(L, qkv, mask, c0, l0, dctx, B, S, nh))


@pytest.mark.parametrize("S,nh", [(37, 12), (129, 16), (266, 12)])
def test_mha_dropout_matches_the_replayed_mask(L, S, nh):
    """the kept / dropped pattern and the 1/(1-p) scale are tests/dropout_replay.attn_mask's; backward through that mask"""
    B, p, seed = 4, 0.1, 0x1234567890AB
    qkv, mask, H = _inputs(B, S, nh, seed=7 + S, scale=0.7)
    keep = attn_mask(seed, B, nh, S, p).to(DEV)
    assert 0.85 < (keep > 0).float().mean().item() < 0.95
    ctx, lse = _fwd(L, qkv, mask, B, S, nh, p_drop=p, seed=seed)
    qf = qkv.float().requires_grad_(True)
    ref, rlse = _ref(qf, mask, B, S, nh, keep=keep)
    close(heads(ctx.float(), B, S, nh), ref.detach(), 2e-2, 2e-2, "ctx with dropout")
    close(lse, rlse.detach(), 1e-3, 1e-3, "lse (before dropout)")
    ctx0, _ = _fwd(L, qkv, mask, B, S, nh)
    assert (ctx0.float() - ctx.float()).abs().max().item() > 1e-2  # dropout did something
    dctx = torch.randn(B * S, H, generator=torch.Generator().manual_seed(3)).to(BF16).to(DEV)
    (unheads(ref) * dctx.float()).sum().backward()
    dqkv = _bwd(L, qkv, mask, ctx, lse, dctx, B, S, nh, p_drop=p, seed=seed)
    sc = qf.grad.abs().max().item()
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)), ("dV", slice(2 * H, 3 * H))):
        close(dqkv[:, sl], qf.grad[:, sl], 3e-2, 2e-2 * sc, f"{name} with dropout")
    # the device seed word is added to the launch-time seed (captured launches draw fresh masks per replay)
    from frozenbilm_amd import lib

    word = torch.tensor([5], dtype=torch.int64, device=DEV)
    with lib.seed_word(word):
        c5, _ = _fwd(L, qkv, mask, B, S, nh, p_drop=p, seed=seed - 5)
    assert torch.equal(c5, ctx)


def test_mha_graph_replay_equals_eager(L):
    B, S, nh = 4, 74, 12
    qkv, mask, H = _inputs(B, S, nh, seed=5, scale=0.7)
    dctx = torch.randn(B * S, H, generator=torch.Generator().manual_seed(9)).to(BF16).to(DEV)
    kl = _klen(mask)
    ctx = torch.empty(B * S, H, dtype=BF16, device=DEV)
    lse = torch.empty(B, nh, S, device=DEV)
    Dv = torch.empty(B, nh, S, device=DEV)
    dqkv = torch.empty(B * S, 3 * H, dtype=BF16, device=DEV)

    def step():
        L.mha_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], mask.view(-1), SCALE, ctx, lse, B, S, nh, p_drop=0.1, seed=11,
                  klen=kl)
        L.attn_rowdot(dctx, ctx, Dv, B, S, nh)
        L.mha_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], dctx, mask.view(-1), lse, Dv, SCALE, dqkv[:, :H],
                  dqkv[:, H:2 * H], dqkv[:, 2 * H:], B, S, nh, p_drop=0.1, seed=11, klen=kl)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = (ctx.clone(), lse.clone(), dqkv.clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in (ctx, lse, dqkv):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, (ctx, lse, dqkv)):
        assert torch.equal(a, b)


def test_mha_refuses_bad_shapes(L):
    """S > 512 (the reference's position table) and misaligned row strides are argument errors, not launches"""
    qkv, mask, H = _inputs(1, 16, 12, seed=1)
    ctx = torch.empty(16, H, dtype=BF16, device=DEV)
    lse = torch.empty(1, 12, 16, device=DEV)
    lib = L.load()
    p = qkv.data_ptr()
    args = lambda S, ld: (p, ld, p, ld, p, ld, mask.data_ptr(), None, None, SCALE, 0.0, 0, None, ctx.data_ptr(), H,
                          lse.data_ptr(), 1, S, 12, None)
    assert lib.fbl_mha_fwd(*args(513, 3 * H)) == -1
    assert lib.fbl_mha_fwd(*args(16, 3 * H + 4)) == -2
    torch.cuda.synchronize()
