"""GPU: the disentangled attention on selected query rows (fbl_disent_attn_fwd_qrows / _bwd_qrows, include/fbl_qrows.h) against
tests/gpu_refs.ref_attention on the full grid read at the selected rows, and against the shipped full-grid kernels.

Inputs as tests/test_gpu_kernels._attn_inputs builds them (the backward comparisons scale q, k, v and the tables by 0.5, as
test_attention_bwd does); the bounds are those of test_attention_fwd / test_attention_bwd.  B = 4, nh = 2:
  sample 0: 17 selected rows (positions 0, klen - 1, one masked position and 14 others), its last 5 positions masked,
  sample 1: every position selected, a hole in its mask (mask[1, 1:3] = 0: two masked query rows, two masked keys),
  sample 2: no selected row, klen = 20,
  sample 3: one selected row.
S = 37 (one partial key tile), 140 (the |delta| >= 128 log buckets), 512 (the table edge); each on the grid and on a row0 layout.
The reference of one S is computed once and shared."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_refs import bf, heads, ref_attention, stats, unheads  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
B, NH, H = 4, 2, 128
SCALE = 1 / math.sqrt(192)
SIZES = [37, 140, 512]


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


def close(got, ref, rtol, atol, name=""):
    print(stats(name, got.float(), ref.float()))
    assert torch.allclose(got.float(), ref.float(), rtol=rtol, atol=atol), stats(name, got.float(), ref.float())


def _ref(qkv, pqk, relidx, mask, S, dctx=None, keep=None):
    """ctx [B*S, H] and lse [B, nh, S] of the full grid; with dctx also the gradients of qkv and pqk"""
    qkvf, pqkf = qkv.float().requires_grad_(dctx is not None), pqk.float().requires_grad_(dctx is not None)
    q, k, v = (heads(qkvf[:, i * H:(i + 1) * H], B, S, NH) for i in range(3))
    pq = pqkf[:, :H].view(-1, NH, 64).permute(1, 0, 2)
    pk = pqkf[:, H:].view(-1, NH, 64).permute(1, 0, 2)
    ctx, lse = ref_attention(q, k, v, pk, pq, relidx, mask, SCALE, drop_keep=keep)
    ctx = unheads(ctx)
    if dctx is None:
        return ctx.detach(), lse.detach(), None, None
    (ctx * dctx.float()).sum().backward()
    return ctx.detach(), lse.detach(), qkvf.grad, pqkf.grad


@functools.lru_cache(maxsize=None)
def case(S):
    from frozenbilm_amd.row_plan import plan_query_rows
    from tests.test_gpu_kernels import _attn_inputs, _klen, rnd

    qkv, pqk, mask, relidx, h = _attn_inputs(B, S, NH, seed=40 + S)
    assert h == H and mask[0, S - 5:].sum() == 0 and mask[1, 1:3].sum() == 0
    mask[2, 20:] = 0
    g = torch.Generator().manual_seed(S)
    others = (torch.randperm(S - 7, generator=g)[:14] + 1).tolist()  # distinct positions in [1, S - 7]
    rows = [0, S - 6, S - 5] + others                    # sample 0: first, klen - 1, a masked position, 14 more
    rows += [S + s for s in range(S)]                    # sample 1: all
    rows += [3 * S + S // 2]                             # sample 3: one
    rows = torch.tensor(rows)[torch.randperm(len(rows), generator=g)].to(DEV)
    klen = _klen(mask)
    assert klen.tolist() == [S - 5, S, 20, S]
    plen = [S - 4, S, 20, S]                             # packed layout: every valid and every selected position has a row
    sel = torch.cat([b * S + torch.arange(n) for b, n in enumerate(plen)]).to(DEV)
    inv = torch.full((B * S,), -1, dtype=torch.int64, device=DEV)
    inv[sel] = torch.arange(sel.numel(), device=DEV)
    row0 = torch.tensor([0] + list(torch.tensor(plen).cumsum(0)), dtype=torch.int32, device=DEV)
    plan = plan_query_rows(rows, B, S)
    assert torch.equal(plan_query_rows(rows, B, S, inv=inv).krows, inv[plan.grid]) and (inv[plan.grid] >= 0).all()
    dctx = torch.zeros(B * S, H, dtype=BF16, device=DEV)
    dctx[plan.grid] = bf(rnd(B * S, H, seed=5)).to(BF16)[plan.grid]
    c = dict(S=S, Sp=(S + 63) // 64 * 64, qkv=qkv, pqk=pqk, mask=mask, relidx=relidx, klen=klen, rows=rows, plan=plan, sel=sel,
             row0=row0, dctx=dctx, span2=pqk.shape[0])
    c["ref_ctx"], c["ref_lse"], _, _ = _ref(qkv, pqk, relidx, mask, S)
    c["qkv_h"], c["pqk_h"] = (qkv.float() * 0.5).to(BF16), (pqk.float() * 0.5).to(BF16)  # the backward's operands
    _, _, c["g_qkv"], c["g_pqk"] = _ref(c["qkv_h"], c["pqk_h"], relidx, mask, S, dctx=dctx)
    return c


def run_fwd(L, c, qkv, pqk, packed, p_drop=0.0, seed=0):
    pl, S = c["plan"], c["S"]
    kv = qkv[c["sel"]].contiguous() if packed else qkv
    q = qkv[pl.grid, :H].contiguous()
    ctx = torch.full((pl.R, H), float("nan"), dtype=BF16, device=DEV)
    lse = torch.full((NH, pl.R), float("nan"), dtype=F32, device=DEV)
    L.disent_attn_fwd_qrows(q, pl.rseg, pl.rpos, kv[:, H:2 * H], kv[:, 2 * H:], pqk[:, H:], pqk[:, :H], c["relidx"], c["mask"].view(-1),
                            c["klen"], SCALE, ctx, lse, B, S, c["Sp"], NH, c["span2"], p_drop=p_drop, seed=seed,
                            row0=c["row0"] if packed else None)
    return q, kv, ctx, lse


def run_bwd(L, c, qkv, pqk, packed, p_drop=0.0, seed=0):
    """forward + backward on NaN-filled outputs -> dict of everything the two calls wrote"""
    pl, S = c["plan"], c["S"]
    q, kv, ctx, lse = run_fwd(L, c, qkv, pqk, packed, p_drop, seed)
    nan = lambda *shape, dtype=BF16: torch.full(shape, float("nan"), dtype=dtype, device=DEV)  # noqa: E731
    dQ, dKV = nan(pl.R, H), nan(kv.shape[0], 2 * H)
    dPK, dPQ = nan(NH, c["span2"], 64, dtype=F32), nan(NH, c["span2"], 64, dtype=F32)
    ws = torch.full((L.disent_attn_bwd_qrows_ws_bytes(pl.R, c["Sp"], NH),), 0xFF, dtype=torch.uint8, device=DEV)
    dO = c["dctx"][pl.grid].contiguous()
    L.disent_attn_bwd_qrows(q, pl.rseg, pl.rpos, kv[:, H:2 * H], kv[:, 2 * H:], pqk[:, H:], pqk[:, :H], c["relidx"], c["mask"].view(-1),
                            c["klen"], dO, ctx, lse, SCALE, dQ, dKV[:, :H], dKV[:, H:], dPK, dPQ, 0, c["span2"], ws, B, S, c["Sp"], NH,
                            c["span2"], p_drop=p_drop, seed=seed, row0=c["row0"] if packed else None)
    rows_t = lambda t: t.permute(1, 0, 2).reshape(c["span2"], H)  # noqa: E731  [nh, w, 64] -> [w, nh*64]
    return dict(ctx=ctx, lse=lse, dQ=dQ, dK=dKV[:, :H], dV=dKV[:, H:], dPK=rows_t(dPK), dPQ=rows_t(dPQ))


def _masked_query(c):
    pl, S = c["plan"], c["S"]
    return c["mask"].view(-1)[pl.grid] == 0


@pytest.mark.parametrize("packed", [False, True], ids=["grid", "row0"])
@pytest.mark.parametrize("S", SIZES)
def test_forward_against_reference(L, S, packed):
    c = case(S)
    pl = c["plan"]
    _, _, ctx, lse = run_fwd(L, c, c["qkv"], c["pqk"], packed)
    close(ctx, c["ref_ctx"][pl.grid], 2e-2, 2e-2, f"ctx S={S}")
    dead = _masked_query(c)
    assert int(dead.sum()) == 3  # one in sample 0, the two of the hole in sample 1
    b_of, pos = pl.grid // S, pl.grid % S
    ref_lse = c["ref_lse"][b_of, :, pos].t()  # [nh, R]
    close(lse[:, ~dead], ref_lse[:, ~dead], 1e-3, 1e-3, "lse")
    assert torch.isinf(lse[:, dead]).all() and (ctx[dead] == 0).all()  # the masked query rows are exactly zero
    assert torch.isfinite(ctx.float()).all()


@pytest.mark.parametrize("packed", [False, True], ids=["grid", "row0"])
@pytest.mark.parametrize("S", SIZES)
def test_backward_against_autograd_and_bit_identical(L, S, packed):
    c = case(S)
    pl = c["plan"]
    out = run_bwd(L, c, c["qkv_h"], c["pqk_h"], packed)
    again = run_bwd(L, c, c["qkv_h"], c["pqk_h"], packed)
    for n, t in out.items():
        fin = torch.isfinite(t.float())
        if n == "lse":
            fin = fin | torch.isinf(t) & _masked_query(c)[None]
        assert fin.all(), n                                   # the outputs started NaN-filled
        assert torch.equal(t.view(torch.int16 if t.dtype == BF16 else torch.int32),
                           again[n].view(torch.int16 if t.dtype == BF16 else torch.int32)), n  # two identical calls: same bits
    g, gp = c["g_qkv"], c["g_pqk"]
    keyrows = c["sel"] if packed else torch.arange(B * S, device=DEV)
    sc, sp = g.abs().max().item(), gp.abs().max().item()
    close(out["dQ"], g[pl.grid, :H], 3e-2, 2e-2 * sc, "dQ")
    close(out["dK"], g[keyrows, H:2 * H], 3e-2, 2e-2 * sc, "dK")
    close(out["dV"], g[keyrows, 2 * H:], 3e-2, 2e-2 * sc, "dV")
    close(out["dPK"], gp[:, H:], 3e-2, 2e-2 * sp, "dPK")
    close(out["dPQ"], gp[:, :H], 3e-2, 2e-2 * sp, "dPQ")
    # exact zeros: masked query rows, masked keys, keys beyond klen, and every row of the sample without a selected row
    assert (out["dQ"][_masked_query(c)] == 0).all()
    zero_key = (c["mask"].view(-1) == 0) | (torch.arange(B * S, device=DEV) // S == 2)
    assert (out["dK"][zero_key[keyrows]] == 0).all() and (out["dV"][zero_key[keyrows]] == 0).all()
    assert (out["dK"][~zero_key[keyrows]] != 0).any()


@pytest.mark.parametrize("packed", [False, True], ids=["grid", "row0"])
@pytest.mark.parametrize("p_drop,seed", [(0.0, 0), (0.1, 7)], ids=["p0", "p0.1"])
@pytest.mark.parametrize("S", SIZES)
def test_against_the_full_grid_kernels(L, S, p_drop, seed, packed):
    """fbl_disent_attn_fwd with saved probabilities -> disent_attn_bwd, fed dO that is zero off the selected rows.  The dropout
    mask is keyed by positions, so with p = 0.1 both sides drop the same pairs."""
    from tests.test_gpu_kernels import _attn_bwd_call, _run_attn_fwd

    c = case(S)
    pl = c["plan"]
    qkv, pqk = c["qkv_h"], c["pqk_h"]
    saved = []
    ctx_f, lse_f = _run_attn_fwd(L, qkv, pqk, c["mask"], c["relidx"], B, S, NH, p_drop=p_drop, seed=seed, save_p=saved)
    dqkv, dpqk = _attn_bwd_call(L, qkv, pqk, ctx_f, lse_f, c["dctx"], c["mask"], c["relidx"], B, S, NH, H, p_drop, seed, saved=saved)
    out = run_bwd(L, c, qkv, pqk, packed, p_drop, seed)  # (the full-grid side stays on the grid: read at the rows that exist)
    keyrows = c["sel"] if packed else torch.arange(B * S, device=DEV)
    close(out["ctx"], ctx_f[pl.grid], 2e-2, 2e-2, "ctx")
    dead = _masked_query(c)
    b_of, pos = pl.grid // S, pl.grid % S
    close(out["lse"][:, ~dead], lse_f[b_of, :, pos].t()[:, ~dead], 1e-3, 1e-3, "lse")
    sc, sp = dqkv.float().abs().max().item(), dpqk.float().abs().max().item()
    close(out["dQ"], dqkv[pl.grid, :H], 3e-2, 2e-2 * sc, "dQ")
    close(out["dK"], dqkv[keyrows, H:2 * H], 3e-2, 2e-2 * sc, "dK")
    close(out["dV"], dqkv[keyrows, 2 * H:], 3e-2, 2e-2 * sc, "dV")
    close(out["dPK"], dpqk[:, H:], 3e-2, 2e-2 * sp, "dPK")
    close(out["dPQ"], dpqk[:, :H], 3e-2, 2e-2 * sp, "dPQ")


def test_dropout_rate_and_no_rows(L):
    """q = k = 0, tables 0, v = 1, p = 0.1: ctx = the kept share / (1 - p) ~ 1 and not constant; R = 0 launches nothing"""
    from frozenbilm_amd.row_plan import plan_query_rows
    from tests.test_gpu_kernels import _attn_inputs

    S = 128
    qkv, pqk, mask, relidx, _ = _attn_inputs(1, S, 1, seed=3)
    mask[:] = 1
    qkv[:, :128] = 0
    pqk[:] = 0
    qkv[:, 128:] = 1.0
    klen = torch.full((1,), S, dtype=torch.int32, device=DEV)
    for rows in (torch.arange(S, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV)):
        pl = plan_query_rows(rows, 1, S)
        ctx = torch.full((pl.R, 64), float("nan"), dtype=BF16, device=DEV)
        lse = torch.empty(1, pl.R, device=DEV)
        L.disent_attn_fwd_qrows(qkv[pl.grid, :64].contiguous(), pl.rseg, pl.rpos, qkv[:, 64:128], qkv[:, 128:], pqk[:, 64:], pqk[:, :64],
                                relidx, mask.view(-1), klen, SCALE, ctx, lse, 1, S, S, 1, pqk.shape[0], p_drop=0.1, seed=5)
        if pl.R:
            m = ctx.float().mean().item()
            assert abs(m - 1.0) < 0.02, m
            assert ctx.float().std().item() > 1e-3


def test_duplicate_rows_and_a_table_sub_range(L):
    """A position selected twice gives the same bits twice (forward), and the gradients of the table rows rmin .. rmin + rcnt - 1
    alone are the same bits as those rows of the whole table (every table row has its own writer)."""
    from frozenbilm_amd.row_plan import plan_query_rows

    c = dict(case(140))
    S = c["S"]
    rows = torch.tensor([S + 7, 3 * S + 70, S + 7, 5, 3 * S + 70, S + 139], device=DEV)  # caller order: duplicates, unsorted
    c["plan"] = pl = plan_query_rows(rows, B, S)
    c["dctx"] = torch.zeros_like(c["dctx"])
    c["dctx"][pl.grid] = 0.25
    _, _, ctx, lse = run_fwd(L, c, c["qkv"], c["pqk"], False)
    back = ctx[pl.back]  # the caller's order
    assert torch.equal(back[0], back[2]) and torch.equal(back[1], back[4]) and not torch.equal(back[0], back[1])
    close(back, c["ref_ctx"][rows], 2e-2, 2e-2, "ctx, caller order")
    whole = run_bwd(L, c, c["qkv_h"], c["pqk_h"], False)
    # the same call for the table rows [100, 400)
    q, kv, ctx, lse = run_fwd(L, c, c["qkv_h"], c["pqk_h"], False)
    rmin, rcnt = 100, 300
    dQ = torch.empty(pl.R, H, dtype=BF16, device=DEV)
    dKV = torch.empty(B * S, 2 * H, dtype=BF16, device=DEV)
    dPK, dPQ = (torch.full((NH, rcnt, 64), float("nan"), device=DEV) for _ in range(2))
    ws = torch.empty(L.disent_attn_bwd_qrows_ws_bytes(pl.R, c["Sp"], NH), dtype=torch.uint8, device=DEV)
    L.disent_attn_bwd_qrows(q, pl.rseg, pl.rpos, kv[:, H:2 * H], kv[:, 2 * H:], c["pqk_h"][:, H:], c["pqk_h"][:, :H], c["relidx"],
                            c["mask"].view(-1), c["klen"], c["dctx"][pl.grid].contiguous(), ctx, lse, SCALE, dQ, dKV[:, :H], dKV[:, H:],
                            dPK, dPQ, rmin, rcnt, ws, B, S, c["Sp"], NH, c["span2"])
    assert torch.equal(dPK.permute(1, 0, 2).reshape(rcnt, H), whole["dPK"][rmin:rmin + rcnt])
    assert torch.equal(dPQ.permute(1, 0, 2).reshape(rcnt, H), whole["dPQ"][rmin:rmin + rcnt])
    assert torch.equal(dQ, whole["dQ"]) and whole["dPK"].abs().sum() > 0
