"""The checks of tests/test_attn_refs.py (on the fp32 emulation, CPU) and tests/test_gpu_attn_elementwise.py (on the HIP kernels):
what is asserted about the outputs of each attention launch, with the references and judges of tests/attn_refs.py.  A Report
collects the exact checks and the worst |err| / bound of the bounded ones; the tests print it and assert that nothing failed."""
from __future__ import annotations

import math

import torch

from tests.attn_cases import delta_ranges_np, visited_tiles
from tests.attn_refs import (BF16, BF_RND, F16_RND, F64, G_RND, PREFIX_RND, SENT_BF16, SENT_F32, ds_products, expanded_table,
                             inv_keep, judge_ctx, judge_D, judge_dS, judge_dV, judge_lse, judge_P, judge_sum, merge_heads, old_close,
                             recomputed_P, reference, saved_P, split_heads, stage_dspk, widen)


# ------------------------------------------------------------------------------------------------ the checks of a stage
class Report:
    """figures of one run: exact checks (name -> bool) and bounded ones (name -> worst |err| / bound, location)"""

    def __init__(self, tag):
        self.tag, self.exact_, self.bounded_, self.yard = tag, {}, {}, {}

    def exact(self, name, ok):
        self.exact_[name] = bool(ok)

    def bounded(self, name, res):
        self.bounded_[name] = res

    def failed(self):
        return [n for n, ok in self.exact_.items() if not ok] + [n for n, (r, _) in self.bounded_.items() if not r <= 1.0]

    def lines(self):
        out = [f"{self.tag}: exact {n}: {'ok' if ok else 'FAILED'}" for n, ok in self.exact_.items()]
        out += [f"{self.tag}: {n}: worst |err| / bound {r:.3f} at {loc}" for n, (r, loc) in self.bounded_.items()]
        out += [f"{self.tag}: {n}: needs C = {v:.3f}" for n, v in self.yard.items()]
        return out


def check_forward(io, f, keep, rep, saved=True):
    """The forward's outputs f (psave / msave with the sentinel prefill, lse [B,nh,S], ctx rows) against the float64 reference.
    keep: the replayed mask [B, nh, S, S] or None.  Every valid pair / element is judged; masked ones must be exact zeros."""
    x = widen(io, keep)
    r = reference(x, backward=False)
    B, nh, S, Sp = x.B, x.nh, x.S, x.Sp
    qv = x.valid[:, None, :].expand(B, nh, S)
    rep.exact("lse = +inf at masked queries", bool((f.lse[~qv] == float("inf")).all()) and bool(torch.isfinite(f.lse[qv]).all()))
    ctx4 = split_heads(f.ctx, io)
    rep.exact("ctx = 0 at masked queries", bool((ctx4[~qv[..., None].expand_as(ctx4)] == 0).all()))
    (w_, loc), need = judge_lse(f.lse, r, x)
    rep.bounded("lse", (w_, loc)); rep.yard["lse"] = need
    rep.bounded("ctx", judge_ctx(ctx4, r, x))
    if not saved:
        return r, x
    ps = f.psave[:, :, :S, :S]
    bits = f.psave.view(torch.int16)
    if keep is not None:
        want = (keep.to(ps.device) == 0)
        rep.exact("psave sign bit = replayed drop decision", bool(((ps.view(torch.int16) < 0) == want)[x.pair.expand_as(want)].all()))
    else:
        rep.exact("psave sign bit clear without dropout", bool((ps.view(torch.int16) >= 0)[x.pair.expand(B, nh, S, S)].all()))
    ok_zero = ok_sent = ok_ms = True
    for b in range(B):
        nq, nk = visited_tiles(io.case, b)
        rows = x.valid[b].clone()
        rows[nq * 64:] = False
        keys = torch.zeros(Sp, dtype=torch.bool, device=ps.device)
        keys[:nk * 64] = True
        keys[:S] &= ~x.valid[b]                                   # masked keys and, beyond S, the padding keys of visited tiles
        blk = f.psave[b, :, :S][:, rows][:, :, keys]
        ok_zero &= bool((blk == 0).all())
        ok_sent &= bool((bits[b, :, nq * 64:, :] == _i16(SENT_BF16)).all()) and bool((bits[b, :, :, nk * 64:] == _i16(SENT_BF16)).all())
        mb = f.msave.view(torch.int32)[b]
        ok_ms &= bool((mb[:, nk:, :] == SENT_F32).all()) and bool((mb[:, :, nq * 64:] == SENT_F32).all())
        ok_ms &= bool(torch.isfinite(f.msave[b, :, :nk][:, :, rows]).all()) if bool(rows.any()) and nk else True
    rep.exact("psave = +-0 at masked and padding keys", ok_zero)
    rep.exact("unvisited tiles of psave keep the sentinel", ok_sent)
    rep.exact("unvisited tiles of msave keep the sentinel", ok_ms)
    Phat, _ = saved_P(f.psave, f.msave, f.lse, x)
    (w_, loc), need = judge_P(Phat, r, x)
    rep.bounded("P", (w_, loc)); rep.yard["P"] = need
    return r, x


def _i16(v):
    return v - 0x10000 if v > 0x7FFF else v


def check_prep(io, f, Dv, PKX, PQX, rep, QT=None, PQT=None):
    x = widen(io)
    rep.bounded("D", judge_D(Dv, f.ctx, x))
    H = io.H
    if PKX is not None:
        rep.exact("PKX = gathered table", torch.equal(PKX, expanded_table(io.pqk[:, H:], io.relidx, io.S, io.Sp, io.nh)))
    if PQX is not None:
        rep.exact("PQX = gathered table", torch.equal(PQX, expanded_table(io.pqk[:, :H], io.relidx, io.S, io.Sp, io.nh)))
    if QT is not None:
        q4 = torch.zeros(io.B, io.nh, io.Sp, 64, dtype=BF16, device=QT.device)
        q4[:, :, :io.S] = split_heads(io.qkv[:, :H], io, BF16)
        rep.exact("QT = transposed q", torch.equal(QT, q4.permute(1, 3, 0, 2).contiguous()))
        rep.exact("PQT = transposed table", torch.equal(PQT, io.pqk[:, :H].reshape(-1, io.nh, 64).permute(1, 2, 0).contiguous()))


def check_dS_layout(io, dS, dST, rep):
    """dS^T bit-equal to the transpose inside the written corner; exact zeros at masked rows / columns and up to the tile edge"""
    x = widen(io)
    ok_t = ok_z = True
    for b in range(io.B):
        nq, nk = visited_tiles(io.case, b)
        n = nq * 64
        a, t = dS[b, :, :n, :n], dST[b, :, :n, :n]
        ok_t &= torch.equal(a.view(torch.int16), t.transpose(1, 2).view(torch.int16))
        live = torch.zeros(io.Sp, dtype=torch.bool, device=dS.device)
        live[:io.S] = x.valid[b]
        dead = ~live[:n]
        ok_z &= bool((a[:, dead, :] == 0).all()) and bool((a[:, :, dead] == 0).all())
    rep.exact("dS^T = transpose of dS", ok_t)
    rep.exact("dS = 0 at masked rows / columns and up to the tile edge", ok_z)


def check_saved_route(io, f, o, rep, x=None):
    """The saved-P stages, each on its own inputs.  f: the forward's outputs; o: Dv, dS, dST [B,nh,Sp,Sp], dqkv rows, dpos fp32
    [span2, 2H] ([dPQ | dPK])."""
    x = x or widen(io)
    S, H = io.S, io.H
    check_dS_layout(io, o.dS, o.dST, rep)
    Pn, dropped = saved_P(f.psave, f.msave, f.lse, x)
    keep = torch.where(dropped, torch.zeros((), dtype=F64, device=Pn.device), torch.full((), inv_keep(io.p), dtype=F64, device=Pn.device))
    st = stage_dspk(Pn, keep, o.Dv, x)
    lse0 = torch.where(torch.isfinite(f.lse), f.lse, torch.zeros_like(f.lse)).to(F64)
    m = f.msave.to(F64).repeat_interleave(64, dim=2)[:, :, :S, :].transpose(2, 3)
    unit = 1 + torch.where(x.pair, m.abs(), torch.zeros_like(m)) + (lse0.abs() * math.log2(math.e))[..., None]
    (w_, loc), need = judge_dS(o.dS[:, :, :S, :S], st, x, unit)
    rep.bounded("dS", (w_, loc)); rep.yard["dS"] = need
    dQ4, dK4, dV4 = (split_heads(o.dqkv[:, i * H:(i + 1) * H], io) for i in range(3))
    rep.bounded("dV", judge_dV(dV4, st, x))
    _check_from_dS(io, o, rep, x, dQ4, dK4, shear=False)


def _check_from_dS(io, o, rep, x, dQ4, dK4, shear):
    """dQ and dPK from the dS bits, dK and dPQ from the dS^T bits (the saved-P kernel forms dK from the very values it stores as
    dS^T).  shear: dK comes from the recompute route's shear pass, which accumulates G2 in LDS as bf16."""
    S, H = io.S, io.H
    has = torch.zeros(io.B, 1, S, 1, dtype=torch.bool, device=dQ4.device)
    for b in range(io.B):
        has[b, :, :min(io.lens[b], S)] = True
    # (valid pairs only: the rest of the written corner is asserted to be exact zeros, and what lies beyond it is never written
    # -- the sentinel -- and never read)
    zero = torch.zeros((), dtype=F64, device=dQ4.device)
    d = torch.where(x.pair, o.dS[:, :, :S, :S].to(F64), zero)
    dT = torch.where(x.pair, o.dST[:, :, :S, :S].to(F64).transpose(2, 3), zero)    # the dS^T bits, indexed [i, j]
    ax = (x.q.abs(), x.k.abs(), x.pk.abs(), x.pq.abs())
    dQ, _, dPK, _ = ds_products(d, x.q, x.k, x.pk, x.pq, x.R, x.span2)
    mQ, _, mPK, _ = ds_products(d.abs(), *ax, x.R, x.span2)
    _, dK, _, dPQ = ds_products(dT, x.q, x.k, x.pk, x.pq, x.R, x.span2)
    _, mK, _, mPQ, _, G2a = ds_products(dT.abs(), *ax, x.R, x.span2, with_G=True)
    n = 2 * io.Sp
    rep.bounded("dQ", judge_sum(dQ4, dQ, mQ, n, has))
    if shear:
        # a slot of G2 that collects c non-zero values rounds c - 1 partial sums to bf16 (LDS atomics; plain stores where c = 1)
        cnt = ds_products((dT != 0).to(F64), *ax, x.R, x.span2, with_G=True)[5]
        extra = BF_RND * (((cnt - 1).clamp_min(0) * G2a) @ x.pq.abs())
        rep.bounded("dK (shear)", judge_sum(dK4, dK, mK, n, has, extra=extra))
    else:
        rep.bounded("dK", judge_sum(dK4, dK, mK, n, has))
    if getattr(o, "dpos", None) is not None:
        gPQ = o.dpos[:, :H].reshape(-1, io.nh, 64).permute(1, 0, 2)
        gPK = o.dpos[:, H:].reshape(-1, io.nh, 64).permute(1, 0, 2)
        _, _, dcnt = delta_ranges_np(io.case)
        exK = exQ = None
        if int(dcnt.max()) > 8:   # the prefix-difference kernel: G = C(jhi) - C(jlo) of fp32 prefix sums of the whole row
            exK = PREFIX_RND * torch.einsum("bhi,bhid->hd", d.abs().sum(3), ax[0])[:, None, :]
            exQ = PREFIX_RND * torch.einsum("bhj,bhjd->hd", dT.abs().sum(2), ax[1])[:, None, :]
        npos = io.B * io.Sp
        rep.bounded("dPK", judge_sum(gPK, dPK, mPK, npos, None, out_rnd=0.0, operand_rnd=G_RND, extra=exK))
        rep.bounded("dPQ", judge_sum(gPQ, dPQ, mPQ, npos, None, out_rnd=0.0, operand_rnd=G_RND, extra=exQ))


REF_EPS = 1e-10   # what the closed-form float64 reference is itself good for, relative (tests/test_attn_refs.py, against autograd)


def end_to_end_atols(io, keep):
    """(reference dqkv rows, reference dpqk, atol of dqkv, atol of dpqk, which of the two are floors) of the end-to-end check: the
    bound the suite applies at p = 0 (test_gpu_kernels.py::test_attention_bwd), rtol 3e-2 and atol 2e-2 max|ref| over dqkv resp.
    dpqk -- unmodified wherever the reference does not vanish.
    With one key (s1) P = 1 and dS = keep dP - D = 0 identically: the reference of dPK and dPQ is zero, max|ref| is nothing but the
    float64 rounding of the reference itself (below REF_EPS of the sum of the magnitudes of its terms) and the atol means nothing,
    while every bf16 pipeline leaves the residue of the cancelling difference (reference(): dS_noise -- two 64-term fp32 dots, and
    D formed from the bf16 ctx the forward stored).  Only then the atol is the floor: the largest sum|term| of the tensor's
    reductions with that residue in the place of |dS|.  tests/test_attn_refs.py asserts that this happens for dpqk of s1 and
    nowhere else."""
    x = widen(io, keep)
    r = reference(x)
    H = io.H
    ref = torch.cat([merge_heads(t, io) for t in (r.dQ, r.dK, r.dV)], 1)
    rpos = torch.cat([r.dPQ.permute(1, 0, 2).reshape(-1, H), r.dPK.permute(1, 0, 2).reshape(-1, H)], 1)
    mag_qkv = max(t.max().item() for t in (r.dQ_mag, r.dK_mag, r.dV_mag))
    mag_pos = max(r.dPK_mag.max().item(), r.dPQ_mag.max().item())
    vanishes = (ref.abs().max().item() <= REF_EPS * mag_qkv, rpos.abs().max().item() <= REF_EPS * mag_pos)
    atols = [2e-2 * ref.abs().max().item(), 2e-2 * rpos.abs().max().item()]
    if any(vanishes):
        fQ, fK, fPK, fPQ = ds_products(r.dS_noise, x.q.abs(), x.k.abs(), x.pk.abs(), x.pq.abs(), x.R, x.span2)
        if vanishes[0]:
            atols[0] = max(fQ.max().item(), fK.max().item())
        if vanishes[1]:
            atols[1] = max(fPK.max().item(), fPQ.max().item())
    return ref, rpos, atols[0], atols[1], vanishes


def check_end_to_end(io, keep, dqkv, dpqk, rep):
    """the final dqkv rows and dpqk [span2, 2H] ([dPQ | dPK]) against the full float64 reference with the replayed mask"""
    ref, rpos, a0, a1, _ = end_to_end_atols(io, keep)
    H = io.H
    for i, nm in enumerate(("dQ", "dK", "dV")):
        rep.exact(f"end to end {nm}", old_close(dqkv[:, i * H:(i + 1) * H], ref[:, i * H:(i + 1) * H], 3e-2, a0))
    rep.exact("end to end dPQ", old_close(dpqk[:, :H], rpos[:, :H], 3e-2, a1))
    rep.exact("end to end dPK", old_close(dpqk[:, H:], rpos[:, H:], 3e-2, a1))


def check_recompute_route(io, f, o, rep, keep, only_dS=False):
    """The recompute stages: dS against P = exp(s64 - lse_in) with the fp16 term, dV, dQ from the dS bits, the shear pass's dK
    from the dS^T bits, dPK / dPQ from the dS / dS^T bits.  only_dS: the yardstick's call (emulate_ds_recompute)."""
    x = widen(io, keep)
    S, H = io.S, io.H
    if not only_dS:
        check_dS_layout(io, o.dS, o.dST, rep)
    lse0 = torch.where(torch.isfinite(f.lse), f.lse, torch.zeros_like(f.lse))
    P, s, bias = recomputed_P(x, lse0)
    P = torch.where(torch.isfinite(f.lse)[..., None].expand_as(P), P, torch.zeros_like(P))
    kp = x.keep if x.keep is not None else torch.ones_like(P)
    st = stage_dspk(P, kp, o.Dv, x)
    unit = 1 + s.abs() + lse0.to(F64).abs()[..., None]
    fp16_rel = F16_RND * io.scale * bias
    (w_, loc), need = judge_dS(o.dS[:, :, :S, :S], st, x, unit, fp16_rel=fp16_rel)
    rep.bounded("dS (recompute)", (w_, loc)); rep.yard["dS (recompute)"] = need
    if only_dS:
        return
    dQ4, dK4, dV4 = (split_heads(o.dqkv[:, i * H:(i + 1) * H], io) for i in range(3))
    rep.bounded("dV (recompute)", judge_dV(dV4, st, x, extra_mag=(P * kp * fp16_rel).transpose(2, 3) @ x.dO.abs()))
    _check_from_dS(io, o, rep, x, dQ4, dK4, shear=True)
