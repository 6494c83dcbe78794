"""Float64 references, per-element judges and the fp32 yardstick of the fused disentangled-attention kernels (test infrastructure
only: plain torch, device-agnostic, no HIP).  What a test does with them, stage by stage, is tests/attn_checks.py.

    s[i,j] = scale (Q_i.K_j + Q_i.PK[idx(i-j)] + K_j.PQ[idx(i-j)]),  P = softmax_masked(s),  O = (keep * P).V
    D_i = dO_i.O_i,  dP = dO.V^T,  dS = P (keep dP - D) scale,  dV = (keep P)^T.dO
    dQ_i = sum_j dS_ij (K_j + PK[idx(i-j)]),  dK_j = sum_i dS_ij (Q_i + PQ[idx(i-j)])
    dPK[r] = sum_b sum_{idx(i-j) = r} dS_ij Q_i,  dPQ[r] = sum_b sum_{idx(i-j) = r} dS_ij K_j

Everything is computed in closed form (no autograd) from the bf16 input bits, widened and never re-rounded, with an optional
multiplicative keep mask (tests/dropout_replay.attn_mask).  Next to every reduction stands the sum of the magnitudes of its
terms: what the rounding of a sum scales with.

Each stage of the backward is judged ON ITS OWN INPUT BITS, as tests/test_gpu_rowops.py judges its reductions: the reference
of a stage takes what the previous launch really wrote (psave / msave / lse, ctx, Dv, dS, dS^T), so an error is pinned on the
launch that made it and the bound of a stage holds nothing but that stage's own roundings.

Rounding points, as read from the kernel sources (u = 2^-24):
  fp16 T1 / T2     attn_fwd.hip pair1 / pair2 and kernel A of the recompute route (to_f16x4): each bias term of a score is an
                   fp16 value, 2^-11 relative
  bf16 psave       attn_fwd.hip SAVEP: exp2(k2 (s - m)) stored as bf16, 2^-8 relative
  bf16 P operand   pf / pfh of the P.V and dV MFMAs: keep * P rounded to bf16, 2^-8 per term
  bf16 dS          dsb of both kernels A: 2^-8 relative; dK, dQ, dPK, dPQ then read those very bits (no further operand rounding)
  bf16 G           pos_grad: the sheared operand G[r][k] (sum of the deltas of a table row) is rounded to bf16 for the MFMA
  bf16 LDS sums    shear pass of the recompute route: G2 is accumulated in LDS as bf16 (one rounding per added term)
  bf16 outputs     ctx, dQ, dK, dV: 2^-8 relative
  fp32 elsewhere   MFMA accumulation (2 n u sum|term| for n terms), exp2 / log, the D row dot
"""
from __future__ import annotations

import math
import types

import numpy as np
import torch

from tests.attn_cases import visited_tiles

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
U = 2.0 ** -24
BF_RND = 2.0 ** -8     # a correctly rounded bf16 value, relative
F16_RND = 2.0 ** -11   # a correctly rounded fp16 value, relative
# pos_grad: G[r][k] = bf16(fp32 sum of the <= 8 bf16 values of a table row's deltas): 2^-8 + the 8 fp32 additions
G_RND = BF_RND + 2 * 8 * U
# pos_grad, more than 8 deltas on a row: G = bf16(C(jhi) - C(jlo)), C the fp32 prefix sums of the staged row -- each the result of
# at most 24 additions (8 in a chunk, a 3-step scan, the carries of up to 8 chunks, the base): 2 * (2 * 24 u) of the row's sum|x|
PREFIX_RND = 2 * 2 * 24 * U
LOG2E = float(np.float32(1.4426950408889634))
SENT_BF16, SENT_F32 = 0x7FA5, 0x7FC0DEAD   # NaN bit patterns of the sentinel prefill (as in test_gpu_gemm_routes.py)

# Constants of the fp32 terms of the forms of P, lse and dS (the quantities with a transcendental or cancelling step).  The
# yardstick (emulate_fwd / emulate_bwd below: plain fp32 torch with the same rounding points, never the HIP kernel) is
# recomputed by every run and asserted within C / 4; its measured figure is 0.00 in every case -- its error never leaves the
# bf16 / fp16 part of the forms, which is two orders of magnitude above the fp32 part -- so "4 x the yardstick maximum" gives
# no usable constant here and the constants are COUNTS of the fp32 roundings the forms' units stand for instead (counted, not
# measured, and so far never exercised: the kernel's errors do not reach the fp32 term either):
#   C_P    16  score sum (3), k2 scaling + fma (2), exp2 (2 ulp), the stored m k2 and lse (2 + 4),
#              exp2 of their difference when P^ is rebuilt in the judge's float64 from fp32 bits (0): 13 -> 16
#   C_LSE  32  l = sum of 64-key tiles: 16 in-lane additions + 2 shuffles per tile, <= 8 tiles and their alpha rescalings
#              (26 relative roundings of l = absolute ones of log l), m scale (1), logf (2 ulp), the final addition (1): 30 -> 32
#   C_DS   16  exponent m - lse log2 e (2 roundings, each scaled by its term: the unit's 1 + |m| + |lse log2 e|), exp2 (2 ulp),
#              |psave| f (1), dP keep (1), the difference (1), two products (2), the dP dot is separate: 9 -> 16
# Table of the measured figures: tests/test_gpu_attn_elementwise.py.
C_P, C_LSE, C_DS = 16.0, 32.0, 16.0


# ------------------------------------------------------------------------------------------------ layout helpers
def rel_matrix(relidx, S):
    """R[i, j] = idx(i - j): the table row of the pair (query i, key j)"""
    i = torch.arange(S, device=relidx.device)
    return relidx.long()[i[:, None] - i[None, :] + S - 1]


def _row_index(B, S, lens, row0, dev):
    bb, ss, rr = [], [], []
    for b in range(B):
        n = min(lens[b], S)
        bb.append(torch.full((n,), b, dtype=torch.long))
        ss.append(torch.arange(n))
        rr.append(torch.arange(n) + row0[b])
    return torch.cat(bb).to(dev), torch.cat(ss).to(dev), torch.cat(rr).to(dev)


def split_heads(x2d, io, dtype=F64):
    """rows of the case's layout [rows, nh*64] -> [B, nh, S, 64] (positions without an activation row: 0)"""
    bb, ss, rr = _row_index(io.B, io.S, io.lens, io.row0_host, x2d.device)
    out = torch.zeros(io.B, io.S, io.nh, 64, dtype=dtype, device=x2d.device)
    out[bb, ss] = x2d[rr].to(dtype).view(-1, io.nh, 64)
    return out.permute(0, 2, 1, 3).contiguous()


def merge_heads(x4, io):
    """[B, nh, S, 64] -> the rows of the case's layout [rows, nh*64]"""
    bb, ss, rr = _row_index(io.B, io.S, io.lens, io.row0_host, x4.device)
    out = torch.zeros(io.row0_host[-1], io.nh * 64, dtype=x4.dtype, device=x4.device)
    out[rr] = x4.permute(0, 2, 1, 3)[bb, ss].reshape(-1, io.nh * 64)
    return out


def table_heads(t2d, nh, dtype=F64):
    """[span2, nh*64] -> [nh, span2, 64]"""
    return t2d.to(dtype).view(-1, nh, 64).permute(1, 0, 2).contiguous()


def widen(io, keep=None, dtype=F64):
    """The inputs of a case as [B, nh, S, 64] / [nh, span2, 64] tensors of `dtype` (bf16 bits widened) + index helpers.
    keep: [B, nh, S, S] multiplicative dropout mask or None."""
    H = io.H
    x = types.SimpleNamespace(B=io.B, S=io.S, Sp=io.Sp, nh=io.nh, span2=io.span2, scale=io.scale, io=io)
    x.q, x.k, x.v = (split_heads(io.qkv[:, i * H:(i + 1) * H], io, dtype) for i in range(3))
    x.pq, x.pk = table_heads(io.pqk[:, :H], io.nh, dtype), table_heads(io.pqk[:, H:], io.nh, dtype)
    x.dO = split_heads(io.dctx, io, dtype)
    x.R = rel_matrix(io.relidx, io.S)
    x.valid = io.mask.bool()
    # rows that exist in the layout and are valid: a packed sample has rows only below its length
    has = torch.zeros_like(x.valid)
    for b in range(io.B):
        has[b, :min(io.lens[b], io.S)] = True
    x.valid = x.valid & has
    x.pair = x.valid[:, None, :, None] & x.valid[:, None, None, :]   # [B, 1, S, S]
    x.keep = None if keep is None else keep.to(x.q.device).to(dtype)
    return x


def _gather_bias(x, q, k, pk, pq):
    B, nh, S = x.B, x.nh, x.S
    T1 = torch.einsum("bhid,hrd->bhir", q, pk)
    T2 = torch.einsum("bhjd,hrd->bhjr", k, pq)
    c2p = T1.gather(3, x.R.expand(B, nh, S, S))
    p2c = T2.gather(3, x.R.t().expand(B, nh, S, S)).transpose(2, 3)   # [b,h,i,j] = T2[j][idx(i-j)]
    return T1, T2, c2p, p2c


def ds_products(dS, q, k, pk, pq, R, span2, with_G=False):
    """What hangs on dS [B, nh, S(i), S(j)]: (dQ, dK, dPK, dPQ).  With the magnitudes of all arguments it returns the sums of the
    magnitudes of the terms of the same reductions.  with_G: also the sheared sums G1 [B,nh,i,r] and G2 [B,nh,j,r]."""
    B, nh, S, _ = dS.shape
    G1 = torch.zeros(B, nh, S, span2, dtype=dS.dtype, device=dS.device).scatter_add_(3, R.expand(B, nh, S, S), dS)
    G2 = torch.zeros(B, nh, S, span2, dtype=dS.dtype, device=dS.device).scatter_add_(3, R.t().expand(B, nh, S, S), dS.transpose(2, 3))
    dQ = dS @ k + G1 @ pk
    dK = dS.transpose(2, 3) @ q + G2 @ pq
    dPK = torch.einsum("bhir,bhid->hrd", G1, q)
    dPQ = torch.einsum("bhjr,bhjd->hrd", G2, k)
    if with_G:
        return dQ, dK, dPK, dPQ, G1, G2
    return dQ, dK, dPK, dPQ


# ------------------------------------------------------------------------------------------------ the float64 reference
def reference(x, backward=True):
    """Everything of the module docstring in float64 from the widened inputs x (widen(io, keep))."""
    r = types.SimpleNamespace()
    T1, T2, c2p, p2c = _gather_bias(x, x.q, x.k, x.pk, x.pq)
    r.qk = x.q @ x.k.transpose(2, 3)
    r.c2p, r.p2c = c2p, p2c
    r.bias_mag = c2p.abs() + p2c.abs()
    r.s = (r.qk + c2p + p2c) * x.scale
    sm = r.s.masked_fill(~x.pair, float("-inf"))
    lse = torch.logsumexp(sm, -1)
    qv = x.valid[:, None, :].expand_as(lse)
    r.lse = torch.where(qv, lse, torch.full_like(lse, float("inf")))
    r.P = torch.where(x.pair, torch.exp(sm - torch.where(qv, lse, torch.zeros_like(lse))[..., None]), torch.zeros_like(sm))
    keep = x.keep if x.keep is not None else torch.ones_like(r.P)
    r.keep = keep
    r.Pd = r.P * keep
    r.ctx = r.Pd @ x.v
    r.ctx_mag = r.Pd @ x.v.abs()
    if not backward:
        return r
    r.D = (x.dO * r.ctx).sum(-1)
    r.dP = x.dO @ x.v.transpose(2, 3)
    r.dP_mag = x.dO.abs() @ x.v.abs().transpose(2, 3)
    r.dS = r.P * (keep * r.dP - r.D[..., None]) * x.scale
    # the residue any bf16 pipeline leaves in the difference keep dP - D: both are 64-term fp32 dots (2 n u sum|term| each), and
    # D is formed from the ctx the forward STORED, a bf16 value (2^-8 |ctx| per element)
    D_mag = (r.Pd * r.dP_mag).sum(-1)
    D_store = BF_RND * (x.dO.abs() * r.ctx.abs()).sum(-1)
    r.dS_noise = r.P * x.scale * (2 * 64 * U * (keep * r.dP_mag + D_mag[..., None]) + D_store[..., None])
    r.dV = r.Pd.transpose(2, 3) @ x.dO
    r.dV_mag = r.Pd.transpose(2, 3) @ x.dO.abs()
    r.dQ, r.dK, r.dPK, r.dPQ = ds_products(r.dS, x.q, x.k, x.pk, x.pq, x.R, x.span2)
    r.dQ_mag, r.dK_mag, r.dPK_mag, r.dPQ_mag = ds_products(r.dS.abs(), x.q.abs(), x.k.abs(), x.pk.abs(), x.pq.abs(), x.R, x.span2)
    return r


def autograd_reference(x):
    """float64 autograd of the forward formula: what the closed form above must equal"""
    leaves = [t.clone().requires_grad_(True) for t in (x.q, x.k, x.v, x.pk, x.pq)]
    q, k, v, pk, pq = leaves
    _, _, c2p, p2c = _gather_bias(x, q, k, pk, pq)
    s = (q @ k.transpose(2, 3) + c2p + p2c) * x.scale
    s = s.masked_fill(~x.pair, float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(x.pair, p, torch.zeros_like(p))
    if x.keep is not None:
        p = p * x.keep
    ctx = p @ v
    (ctx * x.dO).sum().backward()
    return ctx.detach(), [t.grad for t in leaves]


# ------------------------------------------------------------------------------------------------ stage references
def saved_P(psave, msave, lse, x):
    """(Pn, keep sign) of the saved-P route from the forward's own bits: Pn = |psave| exp2(msave - lse log2 e) on [B, nh, S, S]
    (0 on invalid pairs), dropped = sign bit of psave"""
    S = x.S
    ps = psave[:, :, :S, :S]
    dropped = (ps.view(torch.int16) < 0)
    m = msave.to(F64).repeat_interleave(64, dim=2)[:, :, :S, :]      # [B, nh, j, i]: the maximum of key tile j / 64 for query i
    e = m.transpose(2, 3) - (lse.to(F64) * math.log2(math.e))[..., None]
    Pn = torch.where(x.pair, ps.to(F64).abs() * torch.exp2(torch.where(x.pair, e, torch.zeros_like(e))), torch.zeros_like(e))
    return Pn, dropped


def stage_dspk(Pn, keep, Dv, x):
    """dS, dV (+ magnitudes) of kernel A from ITS inputs: Pn (saved bits or exp(s64 - lse_in)), keep [B,nh,S,S], Dv bits"""
    dP = x.dO @ x.v.transpose(2, 3)
    dP_mag = x.dO.abs() @ x.v.abs().transpose(2, 3)
    D = torch.where(x.valid[:, None, :], Dv.to(F64), torch.zeros_like(Dv, dtype=F64))
    dS = Pn * (keep * dP - D[..., None]) * x.scale
    dS_cancel = Pn * (keep * dP.abs() + D.abs()[..., None]) * x.scale   # what the rounding of the difference scales with
    dS_dot = Pn * keep * dP_mag * x.scale                              # |terms| of the dP row dot
    Pd = Pn * keep
    return types.SimpleNamespace(dS=dS, dS_cancel=dS_cancel, dS_dot=dS_dot, dV=Pd.transpose(2, 3) @ x.dO,
                                 dV_mag=Pd.transpose(2, 3) @ x.dO.abs())


def recomputed_P(x, lse_in):
    """P of the recompute route's kernel A: exp(s64 - lse_in) from q, k and the tables, with the lse bits it is given"""
    _, _, c2p, p2c = _gather_bias(x, x.q, x.k, x.pk, x.pq)
    s = (x.q @ x.k.transpose(2, 3) + c2p + p2c) * x.scale
    e = s - lse_in.to(F64)[..., None]
    P = torch.where(x.pair, torch.exp(torch.where(x.pair, e, torch.zeros_like(e))), torch.zeros_like(e))
    return P, s, (c2p.abs() + p2c.abs())


def stage_from_dS(dS_bits, x):
    """dQ, dK, dPK, dPQ (+ magnitudes) from the dS bits kernel A wrote ([B, nh, S, S] slice, widened)"""
    d = dS_bits.to(F64)
    out = ds_products(d, x.q, x.k, x.pk, x.pq, x.R, x.span2)
    mag = ds_products(d.abs(), x.q.abs(), x.k.abs(), x.pk.abs(), x.pq.abs(), x.R, x.span2)
    return out, mag


def rowdot(ctx_bits2d, x):
    """D and its magnitude sum from the ctx bits and dO"""
    o = split_heads(ctx_bits2d, x.io)
    return (x.dO * o).sum(-1), (x.dO * o).abs().sum(-1)


def expanded_table(tab2d, relidx, S, Sp, nh):
    """PKX / PQX of fbl_attn_bwd_prep: X[h][t] = table[relidx[clamp(t - Sp + S - 1)]] for t in [0, 2 Sp): an exact gather"""
    t = torch.arange(2 * Sp, device=tab2d.device)
    src = relidx.long()[(t - Sp + S - 1).clamp(0, 2 * S - 2)]
    return tab2d.view(-1, nh, 64)[src].permute(1, 0, 2).contiguous()


# ------------------------------------------------------------------------------------------------ judges
def worst(err, bound, where=None):
    """(worst |err| / bound, its index) over the elements `where` selects (all by default); a zero bound admits only a zero error"""
    err = err.abs().to(F64)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.to(F64).clamp_min(1e-300))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    if where is not None:
        ratio = torch.where(where.expand_as(ratio), ratio, torch.zeros_like(ratio))
    if ratio.numel() == 0:
        return 0.0, ()
    flat = int(ratio.argmax())
    return float(ratio.flatten()[flat]), tuple(int(v) for v in np.unravel_index(flat, tuple(ratio.shape)))


def needed_c(err, derived, unit, where=None):
    """the constant C at which |err| <= derived + C unit holds everywhere: the yardstick's figure of a measured bound"""
    need = (err.abs().to(F64) - derived.to(F64)).clamp_min(0) / unit.to(F64).clamp_min(1e-300)
    need = torch.where(err == 0, torch.zeros_like(need), need)
    if where is not None:
        need = torch.where(where.expand_as(need), need, torch.zeros_like(need))
    return float(need.max()) if need.numel() else 0.0


def _P_parts(r, x, fp16_factor):
    """(derived, unit) of a probability: P (2^-8 + f scale (|c2p| + |p2c|)) and u P (1 + |s| + |lse|)"""
    lse = torch.where(torch.isfinite(r.lse), r.lse, torch.zeros_like(r.lse))[..., None]
    derived = r.P * (BF_RND + fp16_factor * x.scale * r.bias_mag)
    unit = U * r.P * (1 + r.s.abs() + lse.abs())
    return derived, unit


def judge_P(Phat, r, x, C=C_P):
    """P^ = |psave| exp2(msave - lse log2 e) against the float64 P on every valid pair:
        |err| <= P (2^-8 [bf16 psave] + 2^-10 scale (|c2p| + |p2c|) [fp16 T1 / T2: the pair's own score and, through lse, its
        row's] + C u (1 + |s| + |lse|) [fp32 scores, exp2, the lse the kernel stored])"""
    derived, unit = _P_parts(r, x, 2 * F16_RND)
    return worst(Phat - r.P, derived + C * unit, x.pair), needed_c(Phat - r.P, derived, unit, x.pair)


def judge_lse(lse, r, x, C=C_LSE):
    """lse against float64: the fp16 roundings of the bias terms move it by their P-weighted mean, the rest is fp32:
        |err| <= 2^-11 scale sum_j P (|c2p| + |p2c|) + C u (1 + |lse| + max_j |s|)"""
    qv = x.valid[:, None, :].expand_as(r.lse)
    ref = torch.where(qv, r.lse, torch.zeros_like(r.lse))
    got = torch.where(qv, lse.to(F64), torch.zeros_like(r.lse))
    derived = F16_RND * x.scale * (r.P * r.bias_mag).sum(-1)
    smax = torch.where(x.pair, r.s.abs(), torch.zeros_like(r.s)).amax(-1)
    unit = U * (1 + ref.abs() + smax)
    return worst(got - ref, derived + C * unit, qv), needed_c(got - ref, derived, unit, qv)


def judge_ctx(ctx4, r, x, C=C_P):
    """ctx [B, nh, S, 64] against float64: every term keep P v carries P's bound (its bf16 MFMA operand instead of psave), the
    sum is an fp32 reduction over the keys (and the tile-wise rescaling: one more rounding per key tile), the output bf16"""
    dP, unit = _P_parts(r, x, 2 * F16_RND)
    perP = (dP + C * unit) * r.keep
    n = x.S + x.Sp // 64
    bound = perP @ x.v.abs() + 2 * n * U * r.ctx_mag + BF_RND * r.ctx.abs()
    return worst(ctx4.to(F64) - r.ctx, bound, x.valid[:, None, :, None])


def judge_D(Dv, ctx_bits2d, x):
    """prep: D against the float64 row dot of the ctx bits and dO: products of bf16 pairs are exact in fp32, 64 additions"""
    ref, mag = rowdot(ctx_bits2d, x)
    has = x.valid[:, None, :]
    return worst(Dv.to(F64) - ref, 2 * 64 * U * mag, has)


def judge_dS(dS_bits, st, x, Pn_unit, fp16_rel=None, C=C_DS):
    """dS against P (keep dP - D) scale of the kernel's own inputs:
        |err| <= 2^-8 |dS| [bf16] + 2 64 u P keep sum|dO v| scale [the dP row dot] + (fp16 term) |dS|
                 + C u P scale (keep |dP| + |D|) Pn_unit    [P = |psave| exp2(m - lse log2 e) resp. exp2(k2 s - lse log2 e), the
                                                             difference and the products in fp32; Pn_unit = 1 + |exponent terms|]"""
    derived = BF_RND * st.dS.abs() + 2 * 64 * U * st.dS_dot
    if fp16_rel is not None:
        derived = derived + fp16_rel * st.dS.abs()
    unit = U * st.dS_cancel * Pn_unit
    err = dS_bits.to(F64) - st.dS
    return worst(err, derived + C * unit, x.pair), needed_c(err, derived, unit, x.pair)


def judge_dV(dV4, st, x, extra_mag=None):
    """dV against sum_i Pn keep dO_i: bf16 operand keep Pn (2^-8 per term) whose fp32 value carries Pn's own roundings
    (C_DS u (1 + |exponent terms|) <= 2^-12 per term: the exponents stay below 2^8; extra_mag: the fp16 term of the recompute
    route, summed per term), fp32 reduction over the queries, bf16 output"""
    n = x.S
    bound = (BF_RND + 2.0 ** -12 + 2 * n * U) * st.dV_mag + BF_RND * st.dV.abs()
    if extra_mag is not None:
        bound = bound + extra_mag
    return worst(dV4.to(F64) - st.dV, bound, x.valid[:, None, :, None])


def judge_sum(got, ref, mag, n, where=None, out_rnd=BF_RND, operand_rnd=0.0, extra=None):
    """a plain fp32 reduction of n exact products: 2 n u sum|term| (+ operand_rnd sum|term| where an operand was rounded, + an
    absolute extra) + the rounding of the output"""
    bound = (2 * n * U + operand_rnd) * mag + out_rnd * ref.abs()
    if extra is not None:
        bound = bound + extra
    return worst(got.to(F64) - ref, bound, where)


def old_close(got, ref, rtol, atol):
    """the global tolerance the suite applied before: torch.allclose on the whole tensor"""
    return bool(torch.allclose(got.to(F64), ref.to(F64), rtol=rtol, atol=atol))


# ------------------------------------------------------------------------------------------------ the fp32 yardstick / emulation
def _bf(t):
    return t.to(BF16).to(F32)


def _f16(t):
    return t.clamp(-65504.0, 65504.0).to(F16).to(F32)


def emulate_fwd(io, keep=None, relidx=None, drop_key=None):
    """The forward in plain fp32 torch with the kernel's documented rounding points: fp32 products, fp16 T1 / T2, the online
    softmax over 64-key tiles in the exp2 domain, bf16 psave with the dropout decision in the sign bit, bf16 P operand, bf16
    ctx.  The yardstick of the measured constants and the honest-rounding witness of the judges.
    relidx: another index vector (a perturbation); drop_key: (b, h, i, j) whose last valid key is left out of the softmax
    (a perturbation) -- see tests/test_attn_refs.py."""
    x = widen(io, keep, F32)
    if relidx is not None:
        x.R = rel_matrix(relidx, io.S)
    B, nh, S, Sp = x.B, x.nh, x.S, x.Sp
    dev = x.q.device
    T1, T2, _, _ = _gather_bias(x, x.q, x.k, x.pk, x.pq)
    c2p = _f16(T1).gather(3, x.R.expand(B, nh, S, S))
    p2c = _f16(T2).gather(3, x.R.t().expand(B, nh, S, S)).transpose(2, 3)
    s = (x.q @ x.k.transpose(2, 3) + c2p) + p2c                     # unscaled, as the kernel keeps them
    kvalid = x.valid[:, None, None, :].expand(B, nh, S, S).clone()
    if drop_key is not None:
        kvalid[drop_key] = False
    s = s.masked_fill(~kvalid, float("-inf"))
    k2 = torch.tensor(io.scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    kp = x.keep if x.keep is not None else torch.ones(B, nh, S, S, dtype=F32, device=dev)
    m_run = torch.full((B, nh, S), float("-inf"), dtype=F32, device=dev)
    l_run = torch.zeros(B, nh, S, dtype=F32, device=dev)
    o = torch.zeros(B, nh, S, 64, dtype=F32, device=dev)
    psave = torch.zeros(B, nh, Sp, Sp, dtype=BF16, device=dev)
    msave = torch.zeros(B, nh, Sp // 64, S, dtype=F32, device=dev)
    for jt in range(Sp // 64):
        j0, j1 = jt * 64, min(jt * 64 + 64, S)
        st = s[..., j0:j1]
        m_new = torch.maximum(m_run, st.amax(-1))
        seen = m_new > float("-inf")
        mk = torch.where(seen, -m_new * k2, torch.zeros_like(m_new))
        p = torch.where(seen[..., None], torch.exp2(st * k2 + mk[..., None]), torch.zeros_like(st))
        alpha = torch.where(seen, torch.exp2(torch.where(seen, (m_run - m_new) * k2, torch.zeros_like(m_new))), torch.ones_like(m_new))
        l_run = l_run * alpha + p.sum(-1)
        m_run = m_new
        kt = kp[..., j0:j1]
        pb = p.to(BF16)
        psave[:, :, :S, j0:j1] = torch.where(kt == 0, -pb, pb)
        msave[:, :, jt] = m_new * k2
        o = o * alpha[..., None] + _bf(p * kt) @ x.v[:, :, j0:j1]
    qv = x.valid[:, None, :].expand(B, nh, S) & (l_run > 0)
    inv = torch.where(qv, 1.0 / torch.where(qv, l_run, torch.ones_like(l_run)), torch.zeros_like(l_run))
    ctx = (o * inv[..., None]).to(BF16)
    lse = torch.where(qv, m_run * io.scale + torch.log(torch.where(qv, l_run, torch.ones_like(l_run))),
                      torch.full_like(l_run, float("inf")))
    # what the kernel leaves untouched: tile pairs it does not visit keep the sentinel
    for b in range(B):
        nq, nk = visited_tiles(io.case, b)
        psave[b, :, nq * 64:, :].view(torch.int16).fill_(SENT_BF16)
        psave[b, :, :, nk * 64:].view(torch.int16).fill_(SENT_BF16)
        msave[b, :, nk:, :].view(torch.int32).fill_(SENT_F32)
        if nq * 64 < S:
            msave[b, :, :, nq * 64:].view(torch.int32).fill_(SENT_F32)
    return types.SimpleNamespace(psave=psave, msave=msave, lse=lse, ctx=merge_heads(ctx, io), x=x)


def emulate_bwd(io, f, p_scaled=True, D_from=None, transpose_tile=None):
    """The saved-P backward (prep, dspk, dq, pos_grad) in plain fp32 torch from the forward outputs f (emulate_fwd or the
    kernel's), with the kernels' rounding points: fp32 D, Pn = |psave| exp2(m - lse log2 e), bf16 dS, bf16 keep P operand of dV,
    bf16 G of pos_grad, bf16 outputs.  p_scaled=False: 1 / (1 - p) missing in keep dP (a perturbation); D_from: ctx bits to form
    D from (a perturbation); transpose_tile: (b, h, it, jt) whose dS^T tile is not the transpose (a perturbation)."""
    x = widen(io, None, F32)
    B, nh, S, Sp = x.B, x.nh, x.S, x.Sp
    ctx_bits = f.ctx if D_from is None else D_from
    D = (x.dO * split_heads(ctx_bits, io, F32)).sum(-1)
    ps = f.psave[:, :, :S, :S]
    dropped = ps.view(torch.int16) < 0
    keep = torch.where(dropped, torch.zeros((), dtype=F32), torch.full((), inv_keep(io.p), dtype=F32)).to(ps.device)
    m = f.msave.repeat_interleave(64, dim=2)[:, :, :S, :].transpose(2, 3)
    live = x.valid[:, None, :].expand(B, nh, S) & torch.isfinite(f.lse)
    e = torch.where(x.pair & live[..., None], m - (f.lse * LOG2E)[..., None], torch.full_like(m, float("-inf")))
    pv = torch.where(x.pair, ps.to(F32).abs(), torch.zeros_like(e)) * torch.exp2(e)
    dP = x.dO @ x.v.transpose(2, 3)
    kdp = dP * keep if p_scaled else dP * (keep != 0).to(F32)
    dS = (pv * (kdp - D[..., None]) * io.scale).to(BF16)
    dV = (_bf(pv * keep).transpose(2, 3) @ x.dO).to(BF16)
    dSf = dS.to(F32)
    dQ, dK, _, _ = ds_products(dSf, x.q, x.k, x.pk, x.pq, x.R, x.span2)
    G1 = torch.zeros(B, nh, S, x.span2, dtype=F32, device=dSf.device).scatter_add_(3, x.R.expand(B, nh, S, S), dSf)
    dPK = torch.einsum("bhir,bhid->hrd", _bf(G1), x.q)
    dS_full = torch.zeros(B, nh, Sp, Sp, dtype=BF16, device=dSf.device)
    dS_full[:, :, :S, :S] = dS
    dST_full = dS_full.transpose(2, 3).contiguous()
    if transpose_tile is not None:
        b, h, it, jt = transpose_tile
        blk = dST_full[b, h, jt * 64:jt * 64 + 64, it * 64:it * 64 + 64]
        dST_full[b, h, jt * 64:jt * 64 + 64, it * 64:it * 64 + 64] = blk.t().clone()
    # what the kernels leave untouched: tile pairs they do not visit keep the sentinel
    for b in range(B):
        n = visited_tiles(io.case, b)[0] * 64
        for t in (dS_full, dST_full):
            t[b, :, n:, :].view(torch.int16).fill_(SENT_BF16)
            t[b, :, :, n:].view(torch.int16).fill_(SENT_BF16)
    # dPQ reads dS^T (fbl_attn_pos_grad, neg = 1) below the samples' lengths
    G2 = torch.zeros(B, nh, S, x.span2, dtype=F32, device=dSf.device).scatter_add_(
        3, x.R.t().expand(B, nh, S, S), torch.where(x.pair, dST_full[:, :, :S, :S].to(F32), torch.zeros((), dtype=F32, device=dSf.device)))
    dPQ = torch.einsum("bhjr,bhjd->hrd", _bf(G2), x.k)
    H = io.H
    dqkv = torch.cat([merge_heads(t.to(BF16), io) for t in (dQ, dK, dV)], 1)
    dpqk = torch.cat([dPQ.permute(1, 0, 2).reshape(-1, H), dPK.permute(1, 0, 2).reshape(-1, H)], 1)
    return types.SimpleNamespace(Dv=D, dS=dS_full, dST=dST_full, dqkv=dqkv, dpqk=dpqk.to(BF16), dpos=dpqk, x=x)


def inv_keep(p):
    """attn_common.h attn_drop_key: the exact 1 / (1 - p_q) of the 16-bit quantised rate"""
    if p <= 0:
        return 1.0
    t = np.float32(p) * np.float32(65536.0) + np.float32(0.5)
    thr = np.float32(np.uint32(min(float(t), 65535.0)))
    return float(np.float32(65536.0) / (np.float32(65536.0) - thr))


def emulate_ds_recompute(io, f, keep, Dv):
    """dS of the recompute route's kernel A in plain fp32 torch from ITS inputs (q, k, tables, the lse and D bits it is given):
    fp16 bias tiles, exp2(k2 s - lse log2 e), bf16 dS.  The yardstick of "dS (recompute)"."""
    x = widen(io, keep, F32)
    B, nh, S, Sp = x.B, x.nh, x.S, x.Sp
    T1, T2, _, _ = _gather_bias(x, x.q, x.k, x.pk, x.pq)
    c2p = _f16(T1).gather(3, x.R.expand(B, nh, S, S))
    p2c = _f16(T2).gather(3, x.R.t().expand(B, nh, S, S)).transpose(2, 3)
    s = (x.q @ x.k.transpose(2, 3) + c2p) + p2c
    k2 = torch.tensor(io.scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    live = x.pair & torch.isfinite(f.lse)[..., None]
    e = torch.where(live, s * k2 - (f.lse * LOG2E)[..., None], torch.full_like(s, float("-inf")))
    p = torch.exp2(e)
    kp = x.keep if x.keep is not None else torch.ones_like(p)
    D = torch.where(x.valid[:, None, :], Dv, torch.zeros_like(Dv))
    dS = torch.zeros(B, nh, Sp, Sp, dtype=BF16, device=p.device)
    dS[:, :, :S, :S] = (p * ((x.dO @ x.v.transpose(2, 3)) * kp - D[..., None]) * io.scale).to(BF16)
    return types.SimpleNamespace(dS=dS, Dv=Dv)
