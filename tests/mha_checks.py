"""The checks of tests/test_mha_refs.py (on the fp32 yardstick, CPU) and tests/test_gpu_mha_elementwise.py (on the HIP kernels):
what is asserted about the outputs of fbl_mha_fwd and fbl_mha_bwd (and of the packed *_rows entries), with the references and
judges of tests/mha_refs.py.  A Report (tests/attn_checks.py) collects the exact checks, the worst |err| / bound of the bounded
ones with its location, and "needs C" per quantity; the tests print it and assert that nothing failed.

Every element of every output is judged: the share left out of the bounded checks is 0.  Masked keys are inside them too --
their reference and their bound are exactly 0, which admits only +-0 -- and are asserted once more by name."""
from __future__ import annotations

import torch

from tests import mha_refs as MR
from tests.attn_checks import REF_EPS, Report  # noqa: F401
from tests.attn_refs import old_close

F64 = torch.float64


def check_forward(io, keep, ctx4, lse, rep):
    """ctx [B, nh, S, 64] (any float dtype) and lse [B, nh, S] of a forward against the float64 reference on the input bits"""
    x = MR.widen(io, keep)
    r = MR.reference(x, backward=False)
    has = x.hasq.expand_as(r.lse)
    rep.exact("lse finite on every row", bool(torch.isfinite(lse[has]).all()))
    rep.exact("ctx finite on every row", bool(torch.isfinite(ctx4.to(F64)[has]).all()))
    w, need = MR.judge_lse(lse, r, x)
    rep.bounded("lse", w); rep.yard["lse"] = need
    w, need = MR.judge_ctx(ctx4, r, x)
    rep.bounded("ctx", w); rep.yard["ctx"] = need
    return r, x


def check_backward(io, keep, lse_bits, ctx2d, D_bits, dQ4, dK4, dV4, rep):
    """D against the row dot of the ctx bits; dQ, dK, dV [B, nh, S, 64] against the float64 backward of THEIR inputs: the lse
    the forward stored and the D that was written.  ctx2d: the ctx rows in the case's layout."""
    x = MR.widen(io, keep)
    rep.bounded("D", MR.judge_D(D_bits, ctx2d, x))
    st = MR.stage_backward(x, lse_bits, D_bits)
    for nm, t, judge in (("dV", dV4, MR.judge_dV), ("dQ", dQ4, MR.judge_dQ), ("dK", dK4, MR.judge_dK)):
        w, need = judge(t, st, x)
        rep.bounded(nm, w); rep.yard[nm] = need
    mk = MR.masked_keys(x)[:, None, :, None]
    rep.exact("dK = +-0 at masked keys", bool((dK4.to(F64)[mk.expand_as(dK4)] == 0).all()))
    rep.exact("dV = +-0 at masked keys", bool((dV4.to(F64)[mk.expand_as(dV4)] == 0).all()))
    # ... where the float64 reference is exactly 0 as well
    rep.exact("reference = 0 at masked keys", bool((st.dK[mk.expand_as(st.dK)] == 0).all()) and bool((st.dV[mk.expand_as(st.dV)] == 0).all()))
    return st, x


def end_to_end_atol(io, keep):
    """(reference dQ, dK, dV [B, nh, S, 64], atol, whether the atol is the floor) of the end-to-end check: the bound the suite
    applies (tests/test_gpu_mha.py: rtol 3e-2, atol 2e-2 max|grad| over dQ, dK and dV together), unmodified wherever the reference
    does not vanish.  With one key (s1) P = 1 and dS = keep dP - D = 0 identically, so dQ = dK = 0 in the reference while every
    bf16 pipeline leaves the residue of the cancelling difference; dV = keep dO does not vanish, so max|grad| still means something
    and the atol stays the suite's.  Only if all three vanished would the atol be the floor, as in
    tests/attn_checks.end_to_end_atols: the largest sum|term| with that residue (two 64-term fp32 dots and the bf16 ctx that D is
    formed from) in the place of |dS|.  tests/test_mha_refs.py asserts that this happens in no case."""
    x = MR.widen(io, keep)
    r = MR.reference(x)
    refs = (r.dQ, r.dK, r.dV)
    top = max(t.abs().max().item() for t in refs)
    mag = max(t.max().item() for t in (r.dQ_mag, r.dK_mag, r.dV_mag))
    if top > REF_EPS * mag:
        return refs, 2e-2 * top, False
    D_mag = (r.Pd * r.dP_mag).sum(-1)
    D_store = MR.BF_RND * (x.dO.abs() * r.ctx.abs()).sum(-1)
    noise = r.P * x.scale * (2 * 64 * MR.U * (r.keep * r.dP_mag + D_mag[..., None]) + D_store[..., None])
    return refs, max((noise @ x.k.abs()).max().item(), (noise.transpose(2, 3) @ x.q.abs()).max().item()), True


def check_end_to_end(io, keep, dQ4, dK4, dV4, rep):
    """the gradients against the full float64 reference (forward errors included) at the suite's own global tolerance"""
    refs, atol, _ = end_to_end_atol(io, keep)
    x = MR.widen(io, None)
    has = x.hasq[..., None]
    for nm, got, ref in zip(("dQ", "dK", "dV"), (dQ4, dK4, dV4), refs):
        got = torch.where(has, got.to(F64), torch.zeros((), dtype=F64, device=ref.device))
        rep.exact(f"end to end {nm}", old_close(got, torch.where(has, ref, torch.zeros_like(ref)), 3e-2, atol))
