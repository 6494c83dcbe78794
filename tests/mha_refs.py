"""Float64 references, per-element judges and the fp32 yardstick of the fused BERT attention (frozenbilm_amd/csrc/mha.hip:
fbl_mha_fwd, fbl_mha_bwd, the packed *_rows entries).  Test infrastructure only: plain torch, device-agnostic, no HIP.  What a
test does with them is tests/mha_checks.py; the cases are tests/mha_cases.py.

    s[i,j] = scale Q_i.K_j + (mask[j] ? 0 : -10000),  lse_i = log sum_j exp s[i,j],  P = exp(s - lse),  ctx = (keep * P).V
    D_i = dO_i.ctx_i,  dP = dO.V^T,  dS = P (keep dP - D) scale,  dV = (keep P)^T.dO,  dQ = dS.K,  dK = dS^T.Q

The mask is additive and on keys only: every query row is computed, and a sample without a valid key softmaxes over all of
its keys with the -10000 as a common offset (lse ~ -1e4).  Everything is closed form (no autograd) from the bf16 input bits,
widened and never re-rounded, with the replayed keep mask of tests/dropout_replay.attn_mask.  Next to every reduction stands
the sum of the magnitudes of its terms.

The forward is judged on the input bits.  The backward is judged ON ITS OWN INPUT BITS, as tests/attn_refs.py judges its
stages: P is rebuilt as exp(s - lse_bits) from the lse the forward really stored, and D is the value fbl_attn_rowdot (or the
rows kernel) really wrote, so the bound of the backward holds nothing but the backward's own roundings and an error of the
forward is pinned on the forward (its lse judge).

Rounding points, as read from mha.hip (u = 2^-24; the subscript 2 marks the exp2 domain: s2 = s log2 e, lse2 = lse log2 e):
  fmaf(sacc, k2, bias)   the score in the exp2 domain, k2 = fl(scale log2 e), bias = 0 or MASK_BIAS = fl(-10000 log2 e):
                         one fp32 rounding AT THE MAGNITUDE OF s2.  On a row without a valid key that is 14427, where the
                         fp32 ulp is 2^-10: every score of such a row sits on a grid of 2^-10 (7e-4 of a probability)
  m_run + log2 l, then * ln 2   the forward's lse: two roundings at |lse2| resp. |lse| (again ~ 1e4 on those rows)
  lse * log2 e           the backward rebuilds P = exp2(fmaf(sacc, k2, bias) - fl(lse log2 e)): one more rounding at 14427
  bf16 P operand         pack_p of the P.V MFMA (forward) and of the dV MFMA: keep * P rounded to bf16, 2^-8 per term
  bf16 dS operand        pack_p of the dK and dQ MFMAs: 2^-8 per term; dS never leaves the registers
  bf16 outputs           ctx, dQ, dK, dV: 2^-8 relative
  fp32 elsewhere         MFMA accumulation, exp2 / log2 (1 ulp), the online-softmax statistics and rescales, the D row dot
"""
from __future__ import annotations

import math
import types

import numpy as np
import torch

from tests.attn_refs import BF_RND, U, judge_D, judge_sum, merge_heads, needed_c, split_heads, worst  # noqa: F401 (re-exported)
from tests.mha_cases import key_tiles

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LOG2E_F = float(np.float32(1.4426950408889634))          # attn_common.h LOG2E
LN2_F = float(np.float32(0.69314718055994531))           # the forward's final factor
MASK_BIAS_F = float(np.float32(-10000.0) * np.float32(LOG2E_F))   # mha.hip MASK_BIAS: fl(-10000 * LOG2E)
LOG2E = math.log2(math.e)

# Constants of the fp32 terms of the forms.  They are COUNTS of the fp32 roundings the forms' units stand for, read from
# mha.hip -- not fitted to the kernel's output.  Every run recomputes the yardstick (emulate_fwd / emulate_bwd below: plain
# fp32 torch with the same rounding points and the same tile-wise online softmax, never the HIP kernel) and asserts it
# within C / 4, the kernel within C.  Table of the measured figures: tests/test_gpu_mha_elementwise.py.
#
#   C    16  a probability (the forms of ctx, dV, dQ, dK), unit u P (1 + |s2| + |lse2|): the two chained MFMA steps of the
#            score (2), k2 = fl(scale log2 e) and the float constant LOG2E (2), MASK_BIAS (1) and the fmaf (1) -- all at
#            |s2| --, fl(lse log2 e) and its constant (2, at |lse2|), the subtraction (1), exp2 (1 ulp = 2 u: 2), the
#            product with keep (1): 12; dS adds fmaf(dP, keep, -D) (1) and the products with P and scale (2): 15 -> 16.
#            (The forward has m_new in the place of lse2 and 1 / l, * inv_l in the place of keep: no more.  The rounding of l
#            itself is an fp32 reduction over the keys and stands in judge_ctx's reduction term.)
#   C_M   8  what scales with |lse| + max_j |s| in lse: at |s|, the score's MFMA steps (2), the two constants of k2 (2),
#            MASK_BIAS (1) and the fmaf (1): 6; at |lse|, m_run + log2 l (1), the constant ln 2 (1) and the final product (1):
#            3.  The unit is the SUM of the two magnitudes, so the larger count stands: 6 -> 8.
#   C_L  64  the absolute part of lse = the relative roundings of l: 16 in-lane additions + 2 shuffles in a tile (18), then for
#            each of the <= 7 later tiles alpha = exp2 (2), l * alpha (1) and the addition (1): 28; the argument and the
#            exp2 of a term (3); log2f, 1 ulp of a value below 9, 2^-20 = 16 u, times ln 2 (11): 60 -> 64.
C, C_L, C_M = 16.0, 64.0, 8.0


# ------------------------------------------------------------------------------------------------ inputs
def widen(io, keep=None, dtype=F64):
    """The inputs of a case as [B, nh, S, 64] tensors of `dtype` (bf16 bits widened; 0 where a packed sample has no row).
    keep: [B, nh, S, S] multiplicative dropout mask or None."""
    x = types.SimpleNamespace(B=io.B, S=io.S, Sp=io.Sp, nh=io.nh, scale=io.scale, io=io)
    x.q, x.k, x.v, x.dO = (split_heads(t, io, dtype) for t in (io.q, io.k, io.v, io.dO))
    dev = x.q.device
    x.kmask = io.mask.bool().to(dev)
    x.has = torch.zeros(io.B, io.S, dtype=torch.bool, device=dev)       # the positions that have an activation row
    for b in range(io.B):
        x.has[b, :io.lens[b]] = True
    x.valid = x.has                                                     # (the name tests/attn_refs.judge_D reads)
    x.hasq = x.has[:, None, :]                                          # [B, 1, S]: per query / per key row of a [B, nh, S] tensor
    x.bias = torch.where(x.kmask, 0.0, -10000.0).to(dtype)              # [B, S], natural domain
    x.keep = None if keep is None else keep.to(dev).to(dtype)
    x.n_red = io.S + io.Sp // 64                                        # an fp32 reduction over the keys / queries + one rounding per tile
    return x


def _scores(x, q, k):
    return (q @ k.transpose(2, 3)) * x.scale + x.bias[:, None, None, :]


# ------------------------------------------------------------------------------------------------ the float64 reference
def reference(x, backward=True):
    """Everything of the module docstring in float64 from the widened inputs x (widen(io, keep))."""
    r = types.SimpleNamespace()
    r.s = _scores(x, x.q, x.k)
    r.lse = torch.logsumexp(r.s, -1)
    r.P = torch.exp(r.s - r.lse[..., None])
    r.keep = x.keep if x.keep is not None else torch.ones_like(r.P)
    r.Pd = r.P * r.keep
    r.ctx = r.Pd @ x.v
    r.ctx_mag = r.Pd @ x.v.abs()
    if not backward:
        return r
    r.D = (x.dO * r.ctx).sum(-1)
    _backward(r, x, r.P, r.D)
    return r


def _backward(r, x, P, D):
    """the backward from a given P and D, with the magnitudes of every reduction"""
    r.dP = x.dO @ x.v.transpose(2, 3)
    r.dP_mag = x.dO.abs() @ x.v.abs().transpose(2, 3)
    r.dS = P * (r.keep * r.dP - D[..., None]) * x.scale
    r.dS_cancel = P * (r.keep * r.dP.abs() + D.abs()[..., None]) * x.scale   # what the rounding of the difference scales with
    r.dS_dot = P * r.keep * r.dP_mag * x.scale                               # |terms| of the dP row dot
    Pd = P * r.keep
    r.dV = Pd.transpose(2, 3) @ x.dO
    r.dV_mag = Pd.transpose(2, 3) @ x.dO.abs()
    r.dQ = r.dS @ x.k
    r.dQ_mag = r.dS.abs() @ x.k.abs()
    r.dK = r.dS.transpose(2, 3) @ x.q
    r.dK_mag = r.dS.abs().transpose(2, 3) @ x.q.abs()


def stage_backward(x, lse_bits, D_bits):
    """The backward's reference on ITS inputs: P = exp(s - lse_bits) with the lse the forward stored, D as it was written.
    Query positions without a row (packed samples) contribute nothing, as in the kernels."""
    st = types.SimpleNamespace()
    st.s = _scores(x, x.q, x.k)
    zero = torch.zeros((), dtype=F64, device=st.s.device)
    st.lse = torch.where(x.hasq, lse_bits.to(F64), zero)
    st.P = torch.where(x.hasq[..., None], torch.exp(st.s - st.lse[..., None]), zero)
    st.keep = x.keep if x.keep is not None else torch.ones_like(st.P)
    st.D = torch.where(x.hasq, D_bits.to(F64), zero)
    _backward(st, x, st.P, st.D)
    return st


def autograd_reference(x):
    """float64 autograd of the forward formula: what the closed form above must equal"""
    q, k, v = (t.clone().requires_grad_(True) for t in (x.q, x.k, x.v))
    p = torch.softmax(_scores(x, q, k), -1)
    if x.keep is not None:
        p = p * x.keep
    ctx = p @ v
    (ctx * x.dO).sum().backward()
    return ctx.detach(), (q.grad, k.grad, v.grad)


# ------------------------------------------------------------------------------------------------ judges
def _P_unit(P, s, lse):
    """u P (1 + |s2| + |lse2|): what one fp32 rounding of a probability's exponent (or of the probability) is worth"""
    return U * P * (1 + (s.abs() + lse.abs()[..., None]) * LOG2E)


def _judge_reduction(got, ref, mag, n, term_derived, term_unit, x):
    """A bf16-rounded fp32 reduction of n terms whose terms carry a bound of their own (term_derived + C term_unit, already summed
    with the magnitude of the other factor): attn_refs.judge_sum with that as the absolute extra, on every row that exists.
    Returns ((worst |err| / bound, index), needs C)."""
    where = x.hasq[..., None]
    w = judge_sum(got, ref, mag, n, where, extra=term_derived + C * term_unit)
    derived = 2 * n * U * mag + BF_RND * ref.abs() + term_derived
    return w, needed_c(got.to(F64) - ref, derived, term_unit, where)


def judge_lse(lse, r, x):
    """lse against float64 on every row:  |err| <= u (C_L + C_M (|lse| + max_j |s|)),  s with the mask bias.  The counts are
    separate: the roundings of the summation are absolute, only those of the score, of m_run + log2 l and of the final product
    scale with |lse|.  On a sample without a valid key this is 8 u 2e4 = 1e-2, where the suite's allclose admits 10.
    Returns ((worst |err| / bound, index), the C_M at which the form holds with C_L in proportion)."""
    unit = U * (C_L + C_M * (r.lse.abs() + r.s.abs().amax(-1)))
    w = worst(lse.to(F64) - r.lse, unit, x.hasq)
    return w, w[0] * C_M


def judge_ctx(ctx4, r, x):
    """ctx [B, nh, S, 64] against float64:
        |err| <= sum_j keep |v| P (2^-8 [bf16 P operand] + C u (1 + |s2| + |lse2|)) + 2 (2 n) u sum|term| + 2^-8 |ctx|
    n = S + Sp / 64: the numerator o and the denominator l are each an fp32 reduction over the keys with one more rounding
    (the alpha rescale) per key tile"""
    return _judge_reduction(ctx4, r.ctx, r.ctx_mag, 2 * x.n_red, (BF_RND * r.Pd) @ x.v.abs(),
                            (_P_unit(r.P, r.s, r.lse) * r.keep) @ x.v.abs(), x)


def judge_dV(dV4, st, x):
    """dV against sum_i P keep dO_i, P = exp(s - lse_bits):
        |err| <= sum_i keep |dO| P (2^-8 + C u (1 + |s2| + |lse2|)) + 2 n u sum|term| + 2^-8 |dV|
    A masked key of a sample with a valid key has P = 0 in float64 too: the bound is 0 and admits only +-0."""
    return _judge_reduction(dV4, st.dV, st.dV_mag, x.n_red, (BF_RND * st.P * st.keep).transpose(2, 3) @ x.dO.abs(),
                            (_P_unit(st.P, st.s, st.lse) * st.keep).transpose(2, 3) @ x.dO.abs(), x)


def _dS_parts(st):
    """(derived, unit) of one dS term: 2^-8 |dS| [bf16 operand] + 2 64 u P keep sum|dO v| scale [the dP dot]  and
    u P scale (keep |dP| + |D|) (1 + |s2| + |lse2|) [P's exponent, exp2, the difference and the products in fp32]"""
    derived = BF_RND * st.dS.abs() + 2 * 64 * U * st.dS_dot
    unit = U * st.dS_cancel * (1 + (st.s.abs() + st.lse.abs()[..., None]) * LOG2E)
    return derived, unit


def judge_dQ(dQ4, st, x):
    """dQ against sum_j dS K_j: the per-term dS bound times |K|, the fp32 reduction over the keys, the bf16 output"""
    d, un = _dS_parts(st)
    return _judge_reduction(dQ4, st.dQ, st.dQ_mag, x.n_red, d @ x.k.abs(), un @ x.k.abs(), x)


def judge_dK(dK4, st, x):
    """dK against sum_i dS Q_i: the per-term dS bound times |Q|, the fp32 reduction over the queries, the bf16 output"""
    d, un = _dS_parts(st)
    return _judge_reduction(dK4, st.dK, st.dK_mag, x.n_red, d.transpose(2, 3) @ x.q.abs(), un.transpose(2, 3) @ x.q.abs(), x)


def masked_keys(x):
    """[B, S]: the masked keys of the samples that have a valid key -- where dK = dV = +-0 exactly (P = exp2(.. - 14427) = 0 in
    fp32, exp(-10000) = 0 in float64).  The key tiles beyond klen are among them."""
    return ~x.kmask & x.kmask.any(1, keepdim=True) & x.has


# ------------------------------------------------------------------------------------------------ the fp32 yardstick
def _bf(t, trunc=False):
    if trunc:
        return (t.contiguous().view(torch.int32) & -65536).view(F32)
    return t.to(BF16).to(F32)


def _fmaf(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 values is exact in float64, the sum is rounded once more on the way back"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _scores2(x, io, b):
    """fmaf(sacc, k2, bias) of sample b in the exp2 domain, [nh, S, S] fp32"""
    k2 = torch.tensor(io.scale, dtype=F32) * torch.tensor(LOG2E_F, dtype=F32)
    sacc = x.q[b] @ x.k[b].transpose(1, 2)
    bias = torch.where(x.kmask[b], 0.0, MASK_BIAS_F).to(F32)
    return _fmaf(sacc, k2.to(sacc.device), bias[None, None, :])


def emulate_fwd(io, keep=None, ignore_mask=None, no_alpha=False, exp_bias=0.0, trunc=False):
    """The forward in plain fp32 torch with mha.hip's rounding points: the fmaf of the score, the online softmax over the
    visited 64-key tiles in the exp2 domain, the bf16 keep * P operand, o / l in fp32, bf16 ctx, lse = (m + log2 l) ln 2.
    Returns ctx [B, nh, S, 64] bf16 and lse [B, nh, S] fp32.
    Wrong variants (tests/test_mha_refs.py): ignore_mask = (b, j): that mask zero is taken for a one; no_alpha: the rescale
    of l and o between tiles left out; exp_bias: every exp2 of a score high by that factor; trunc: the bf16 operand truncated."""
    if ignore_mask is not None:
        io = types.SimpleNamespace(**vars(io))
        io.mask = io.mask.clone()
        io.mask[ignore_mask] = 1
    x = widen(io, keep, F32)
    B, nh, S = x.B, x.nh, x.S
    dev = x.q.device
    ctx = torch.zeros(B, nh, S, 64, dtype=BF16, device=dev)
    lse = torch.zeros(B, nh, S, dtype=F32, device=dev)
    for b in range(B):
        pl = io.lens[b]
        t = _scores2(x, io, b)
        kp = x.keep[b] if x.keep is not None else torch.ones(nh, S, S, dtype=F32, device=dev)
        m_run = torch.full((nh, S), float("-inf"), dtype=F32, device=dev)
        l_run = torch.zeros(nh, S, dtype=F32, device=dev)
        o = torch.zeros(nh, S, 64, dtype=F32, device=dev)
        for jt in range(key_tiles(io.kl[b], S, pl)):
            j0, j1 = jt * 64, min(jt * 64 + 64, pl)                 # (keys without a row carry -inf: they add exact zeros)
            tt = t[..., j0:j1]
            m_new = torch.maximum(m_run, tt.amax(-1))
            alpha = torch.ones_like(m_new) if no_alpha else torch.exp2(m_run - m_new)
            p = torch.exp2(tt - m_new[..., None])
            if exp_bias:
                p = p * (1.0 + exp_bias)
            l_run = l_run * alpha + p.sum(-1)
            m_run = m_new
            o = o * alpha[..., None] + _bf(p * kp[..., j0:j1], trunc) @ x.v[b][:, j0:j1]
        ctx[b] = (o * (1.0 / l_run)[..., None]).to(BF16)
        lse[b] = (m_run + torch.log2(l_run)) * LN2_F
    return types.SimpleNamespace(ctx4=ctx, lse=lse)


def emulate_rowdot(io, ctx4):
    """D = dO . ctx of the ctx bits, fp32"""
    x = widen(io, None, F32)
    return (x.dO * ctx4.to(F32)).sum(-1)


def emulate_bwd(io, keep, lse_bits, D_bits, keep_unscaled=False, dq_skips_a_key=False, dk_skips_last_tile=False, trunc=False):
    """The backward (dkdv and dq kernels) in plain fp32 torch from the lse and D bits it is given, with mha.hip's rounding points:
    P = exp2(fmaf(sacc, k2, bias) - fl(lse log2 e)), dS = P fmaf(dP, keep, -D) scale, bf16 keep * P and dS operands, bf16 outputs.
    Returns dQ, dK, dV [B, nh, S, 64] bf16.
    Wrong variants: keep_unscaled: keep dP without the 1 / (1 - p); dq_skips_a_key: key 5 of every tile left out of dQ;
    dk_skips_last_tile: the last query tile left out of dK; trunc: the bf16 operands truncated."""
    x = widen(io, keep, F32)
    B, nh, S = x.B, x.nh, x.S
    dev = x.q.device
    dQ, dK, dV = (torch.zeros(B, nh, S, 64, dtype=BF16, device=dev) for _ in range(3))
    for b in range(B):
        pl = io.lens[b]
        nk = min(key_tiles(io.kl[b], S, pl) * 64, S)              # the keys of the visited tiles; beyond them P = 0
        t = _scores2(x, io, b)
        lse2 = lse_bits[b].to(F32) * LOG2E_F
        p = torch.exp2(t - lse2[..., None])
        live = torch.zeros(S, S, dtype=torch.bool, device=dev)
        live[:pl, :nk] = True
        p = torch.where(live, p, torch.zeros((), dtype=F32, device=dev))
        kf = x.keep[b] if x.keep is not None else torch.ones(nh, S, S, dtype=F32, device=dev)
        dp = x.dO[b] @ x.v[b].transpose(1, 2)
        D = torch.where(x.has[b], D_bits[b].to(F32), torch.zeros((), dtype=F32, device=dev))
        kd = (kf != 0).to(F32) if keep_unscaled else kf
        ds = _bf(p * _fmaf(dp, kd, -D[..., None]) * io.scale, trunc)
        pb = _bf(p * kf, trunc)
        dV[b] = (pb.transpose(1, 2) @ x.dO[b]).to(BF16)
        dsk = ds
        if dk_skips_last_tile:
            dsk = ds.clone()
            dsk[:, (pl - 1) // 64 * 64:, :] = 0
        dK[b] = (dsk.transpose(1, 2) @ x.q[b]).to(BF16)
        dsq = ds
        if dq_skips_a_key:
            dsq = ds.clone()
            dsq[:, :, 5::64] = 0
        dQ[b] = (dsq @ x.k[b]).to(BF16)
    return types.SimpleNamespace(dQ4=dQ, dK4=dK, dV4=dV)
