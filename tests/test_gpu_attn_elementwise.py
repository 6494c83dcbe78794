"""The fused disentangled-attention kernels (csrc/attn_fwd.hip; prep, dspk, ds, dq, shear and pos_grad of csrc/attn_bwd.hip) on the
MI355X, stage by stage and element by element, against the float64 references of tests/attn_refs.py, at the cases of
tests/attn_cases.py, with and without attention dropout (p = 0.1: every training step runs with it).  The dropout masks are
rebuilt on the host (tests/dropout_replay.attn_mask) and applied inside the reference.

The entry points of frozenbilm_amd.lib are driven in the order attn_bwd.disent_attn_bwd uses, and every intermediate is kept:
psave / msave / lse / ctx of the forward, Dv and the expanded tables of prep, dS / dS^T, dV, dK, dQ, dPK, dPQ.  Every stage is
judged on its own input bits (see tests/attn_refs.py), every valid element of every tensor is judged (the share left out is
0; masked elements are covered by exact zeros), and the production sequence run on the same inputs must return the same bits.

Three kinds of assertion, as in tests/test_gpu_rowops.py (u = 2^-24):

(a) Exact.  The sign bit of psave = the replayed drop decision on every valid pair; psave = +-0 at masked and padding keys of valid
    query rows; lse = +inf and ctx = 0 at masked queries; tile pairs the kernels do not visit keep their sentinel; guards intact;
    PKX / PQX = the gather table[relidx[clamp(t - Sp + S - 1)]]; QT / PQT = the torch transposes; dS^T = the transpose of dS inside
    the written corner; dS = 0 at masked rows / columns and between klen and the tile edge; disent_attn_bwd = the stage calls, bit
    for bit.

(b) Derived bounds (constants as they are: 2^-8 a correctly rounded bf16 value, 2^-11 an fp16 one, 2 n u sum|term| an fp32
    reduction of n terms):
      D       2 64 u sum|dO O|
      ctx     sum_j keep |v| bound_P + 2 (S + Sp / 64) u sum|term| + 2^-8 |ctx|
      dV      (2^-8 + 2^-12 + 2 S u) sum|Pn keep dO| + 2^-8 |dV|          (+ sum 2^-11 scale (|c2p| + |p2c|) |term| on the recompute route)
      dQ, dK  2 (2 Sp) u sum|term| + 2^-8 |ref|                           from the dS / dS^T bits: the products are exact
      dK (shear pass)  + 2^-8 sum_r (c - 1) G2abs[j, r] |PQ[r]|            c values accumulated in bf16 in one LDS slot
      dPK, dPQ  (2^-8 + 16 u + 2 B Sp u) sum|term|  (+ 96 u sum_k rowabs_k |y_k| for the prefix-difference kernel)

(c) Forms with an fp32 constant, for what has a transcendental or cancelling step.  The constants are not taken from the HIP kernel:
    every run recomputes the yardstick -- a plain fp32 torch evaluation of the same formula with the same rounding points on the
    same inputs (attn_refs.emulate_fwd / emulate_bwd / emulate_ds_recompute) -- asserts it within C / 4 and the kernel within C.
      P       P (2^-8 + 2^-10 scale (|c2p| + |p2c|) + C u (1 + |s| + |lse|))                      P^ = |psave| exp2(msave - lse log2 e)
      lse     2^-11 scale sum_j P (|c2p| + |p2c|) + C u (1 + |lse| + max_j |s|)
      dS      2^-8 |dS| + 2 64 u P keep sum|dO v| scale + C u P scale (keep |dP| + |D|) (1 + |msave| + |lse log2 e|)
      dS (recompute)  + 2^-11 scale (|c2p| + |p2c|) |dS|, unit (1 + |s| + |lse|)

    "needs C": the smallest C at which the form holds for every element, i.e. how far the error leaves the derived part.

    quantity         yardstick needs C   C     kernel needs C    worst |err| / bound: yardstick   kernel   (at)
    P                0.00                16    0.00              0.980                            0.980    s266p p=0.1
    lse              0.00                32    0.00              0.524                            0.524    s266p p=0.1
    dS               0.00                16    0.00              0.992                            0.992    coarse p=0.1
    dS (recompute)   0.00                16    0.00              0.990                            0.990    clamped p=0.1

    (measured on an MI355X, ROCm 7.0, all cases, p = 0 and 0.1.)  Neither the yardstick nor the kernel ever leaves the bf16 / fp16
    part of the forms -- that part is two orders of magnitude above the fp32 part -- so "4 x the yardstick maximum" gives no usable
    constant; the constants count the fp32 roundings of each form instead (attn_refs.py).  What makes the forms sharp is the
    derived part: 98 - 99 % of the bound is used by honest rounding, and kernel and yardstick agree to the third digit.  The
    fp32 term is thus counted, not measured, and never exercised: no error of the kernel or of the yardstick reaches it.
    Worst |err| / bound of the derived bounds, kernel (yardstick): D 0.006, ctx 0.618 (0.618), dV 0.627 (0.627), dV recompute 0.625, dQ 0.972 (0.972), dK 0.977 (0.966), dK shear pass 0.948, dPK 0.717 (0.659), dPQ 0.810 (0.810);
    fbl_attn_pos_grad on random operands (test_gpu_pos_grad.py) 0.912.

Bit equality with disent_attn_bwd on the recompute route: dS, dS^T, dV, dQ, dPK, dPQ are produced in a fixed order.  The shear
pass's dK is not asserted equal where a table row collects more than one delta: those slots of G2 are summed by LDS atomics
(bf16 additions whose order among the lanes of a wave is the hardware's), so only the bound applies; with one delta per row
(s130) every store is plain and dK must be equal too.
"""
import types

import pytest
import torch

from tests import attn_cases as AC
from tests import attn_checks as CK
from tests import attn_refs as AR
from tests.dropout_replay import attn_mask

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = {F32: AR.SENT_F32, BF16: AR.SENT_BF16}
IVIEW = {F32: torch.int32, BF16: torch.int16}
G = 8  # guard elements / rows


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


# ------------------------------------------------------------------------------------------------ buffers
class Bufs:
    """sentinel-prefilled outputs with guard elements behind them"""

    def __init__(self):
        self.all = []

    def flat(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        full = torch.empty(n + G, dtype=dtype, device=DEV)
        full.view(IVIEW[dtype]).fill_(SENT[dtype])
        self.all.append((full, n))
        return full[:n].view(*shape)

    def rows(self, rows, cols, dtype=BF16):
        full = torch.empty(rows + G, cols, dtype=dtype, device=DEV)
        full.view(IVIEW[dtype]).fill_(SENT[dtype])
        self.all.append((full.view(-1), rows * cols))
        return full[:rows]

    def guards_intact(self):
        return all(bool((full.view(IVIEW[full.dtype])[n:] == SENT[full.dtype]).all()) for full, n in self.all)


def _case(name, p, backward):
    io = AC.make_inputs(name, DEV, backward=backward)
    io.p, io.seed = p, AC.SEED
    keep = attn_mask(io.seed, io.B, io.nh, io.S, p).to(DEV) if p > 0 else None
    H = io.H
    io.q, io.k, io.v = io.qkv[:, :H], io.qkv[:, H:2 * H], io.qkv[:, 2 * H:]
    io.pq, io.pk = io.pqk[:, :H], io.pqk[:, H:]
    return io, keep


def run_fwd(L, io, bufs, save=True):
    f = types.SimpleNamespace(psave=None, msave=None)
    f.ctx = bufs.rows(io.row0_host[-1], io.H)
    f.lse = bufs.flat((io.B, io.nh, io.S), F32)
    if save:
        f.psave = bufs.flat((io.B, io.nh, io.Sp, io.Sp), BF16)
        f.msave = bufs.flat((io.B, io.nh, io.Sp // 64, io.S), F32)
    L.disent_attn_fwd(io.q, io.k, io.v, io.pk, io.pq, io.relidx, io.mask.view(-1), io.scale, f.ctx, f.lse, io.B, io.S, io.Sp,
                      io.nh, io.span2, p_drop=io.p, seed=io.seed, klen=io.klen, border=io.border, lin=io.lin_fwd, row0=io.row0,
                      psave=f.psave, msave=f.msave)
    torch.cuda.synchronize()
    return f


def pos_grads(L, io, dS, dST, bufs):
    """attn_bwd.pos_table_grads, call by call: fp32 [span2, 2H] laid out [dPQ | dPK]"""
    from frozenbilm_amd.attn_bwd import _delta_ranges, _relidx_range

    H, nh = io.H, io.nh
    rmin, rcnt = _relidx_range(io.S, io.cfg)
    dlo, dcnt, cmax = _delta_ranges(io.S, io.cfg, torch.device(DEV), limit=None)
    dpos = torch.zeros(io.span2, 2 * H, dtype=F32, device=DEV)
    for neg, X, Y, col0 in ((0, dS, io.q, H), (1, dST, io.k, 0)):
        d = bufs.flat((1, nh, rcnt, 64), F32)
        L.attn_pos_grad(neg, [X], [Y], dlo, dcnt, cmax, d, io.B, io.S, io.Sp, nh, rcnt, klen=io.klen, row0=io.row0)
        dpos[rmin:rmin + rcnt, col0:col0 + H].view(rcnt, nh, 64).copy_(d[0].permute(1, 0, 2))
    return dpos


def run_bwd_stages(L, io, f, bufs, saved):
    """prep -> dspk -> dq (saved P) or prep -> ds -> dq -> shear (recompute), then pos_grad: lib calls in disent_attn_bwd's order"""
    B, S, Sp, nh, H, span2 = io.B, io.S, io.Sp, io.nh, io.H, io.span2
    o = types.SimpleNamespace(QT=None, PQT=None, PQX=None)
    o.Dv = bufs.flat((B, nh, S), F32)
    o.PKX = bufs.flat((nh, 2 * Sp, 64), BF16)
    if saved:
        o.PQX = bufs.flat((nh, 2 * Sp, 64), BF16)
    else:
        o.QT = bufs.flat((nh, 64, B, Sp), BF16)
        o.PQT = bufs.flat((nh, 64, span2), BF16)
    L.attn_bwd_prep(io.q, io.pq, io.pk, io.dctx, f.ctx, o.QT, o.PQT, o.Dv, B, S, Sp, nh, span2, row0=io.row0, relidx=io.relidx,
                    PQX=o.PQX, PKX=o.PKX)
    o.dS = bufs.flat((B, nh, Sp, Sp), BF16)
    o.dST = bufs.flat((B, nh, Sp, Sp), BF16)
    o.dqkv = bufs.rows(io.row0_host[-1], 3 * H)
    dQ, dK, dV = o.dqkv[:, :H], o.dqkv[:, H:2 * H], o.dqkv[:, 2 * H:]
    lin_a, lin_s = AC.lin_bwd(io.case)
    if saved:
        L.disent_attn_bwd_dspk(f.psave, f.msave, io.q, io.v, io.dctx, o.PQX, f.lse, o.Dv, io.scale, dK, dV, o.dS, o.dST, B, S, Sp, nh,
                               p_drop=io.p, seed=io.seed, klen=io.klen, border=io.border, row0=io.row0)
    else:
        L.disent_attn_bwd_ds(io.q, io.k, io.v, io.dctx, io.pk, io.pq, io.relidx, io.mask.view(-1), f.lse, o.Dv, io.scale, dV, o.dS,
                             o.dST, B, S, Sp, nh, span2, p_drop=io.p, seed=io.seed, klen=io.klen, border=io.border, lin=lin_a,
                             row0=io.row0)
    L.disent_attn_bwd_dq(o.dS, io.k, o.PKX, dQ, B, S, Sp, nh, klen=io.klen, border=io.border, row0=io.row0)
    if not saved:
        L.disent_attn_bwd_shear(o.dST, o.QT, o.PQT, io.relidx, dK, B, S, Sp, nh, span2, klen=io.klen, lin=lin_s, border=io.border,
                                row0=io.row0)
    o.dpos = pos_grads(L, io, o.dS, o.dST, bufs)
    torch.cuda.synchronize()
    return o


def run_production(io, f, saved):
    """attn_bwd.disent_attn_bwd itself on the same inputs (bare stand-ins for the engine's objects)"""
    from frozenbilm_amd.attn_bwd import disent_attn_bwd, pos_table_grads

    eng, run, sv = (types.SimpleNamespace() for _ in range(3))
    eng.H, eng.nh, eng.span2, eng.dev, eng.cfg = io.H, io.nh, io.span2, torch.device(DEV), io.cfg
    eng.relidx = lambda S_: io.relidx
    run.B, run.S, run.mask_i32, run.p_att, run.klen, run.border = io.B, io.S, io.mask.view(-1), io.p, io.klen, io.border
    if io.row0 is not None:
        run.pk = types.SimpleNamespace(row0=io.row0)
    sv.qkv, sv.pqk, sv.ctx, sv.lse, sv.seed_att = io.qkv, io.pqk, f.ctx, f.lse, io.seed
    sv.psave, sv.msave = (f.psave, f.msave) if saved else (None, None)
    dqkv = torch.zeros(io.row0_host[-1], 3 * io.H, dtype=BF16, device=DEV)
    st = disent_attn_bwd(eng, run, sv, io.dctx, dqkv, None, defer_pos=True)
    dpos = pos_table_grads(eng, st)
    torch.cuda.synchronize()
    return types.SimpleNamespace(dS=st["dS"], dST=st["dST"], dqkv=dqkv, dpos=dpos)


def same_corner(io, a, b):
    """dS / dS^T of two runs, bit for bit inside the corner the kernels write (the rest is never written)"""
    ok = True
    for bb in range(io.B):
        n = AC.visited_tiles(io.case, bb)[0] * 64
        ok &= torch.equal(a[bb, :, :n, :n].view(torch.int16), b[bb, :, :n, :n].view(torch.int16))
    return ok


def corner_sentinel(io, t):
    ok = True
    bits = t.view(torch.int16)
    for bb in range(io.B):
        n = AC.visited_tiles(io.case, bb)[0] * 64
        ok &= bool((bits[bb, :, n:, :] == AR.SENT_BF16).all()) and bool((bits[bb, :, :, n:] == AR.SENT_BF16).all())
    return ok


def end_to_end(io, keep, o, rep):
    CK.check_end_to_end(io, keep, o.dqkv, o.dpos.to(BF16), rep)   # (dpqk as disent_attn_bwd stores it: dpqk.copy_(fp32))


def finish(rep, yard=None):
    print("\n".join(rep.lines()))
    if yard is not None:
        print("\n".join(yard.lines()))
        assert yard.failed() == [], yard.failed()
        for n, c in (("P", AR.C_P), ("lse", AR.C_LSE), ("dS", AR.C_DS), ("dS (recompute)", AR.C_DS)):
            if n in yard.yard:
                assert yard.yard[n] <= c / 4, (n, yard.yard[n])
    assert rep.failed() == [], rep.failed()


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("p", AC.P_DROPS)
@pytest.mark.parametrize("name", list(AC.CASES))
def test_forward(L, name, p):
    io, keep = _case(name, p, backward=False)
    bufs = Bufs()
    f = run_fwd(L, io, bufs, save=True)
    rep = CK.Report(f"{name} p={p} kernel")
    CK.check_forward(io, f, keep, rep)
    # the launch without psave (evaluation, and training without attn_save_p): the same lse and ctx bounds
    f2 = run_fwd(L, io, bufs, save=False)
    rep2 = CK.Report(f"{name} p={p} kernel, no psave")
    CK.check_forward(io, f2, keep, rep2, saved=False)
    rep.exact("guards intact", bufs.guards_intact())
    rep.exact("every ctx element written", bool(torch.isfinite(f.ctx).all()) and bool(torch.isfinite(f2.ctx).all()))
    yard = CK.Report(f"{name} p={p} yardstick")
    CK.check_forward(io, AR.emulate_fwd(io, keep), keep, yard)
    finish(rep2)
    finish(rep, yard)


# ------------------------------------------------------------------------------------------------ backward, saved P (shipped)
@pytest.mark.parametrize("p", AC.P_DROPS)
@pytest.mark.parametrize("name", list(AC.CASES))
def test_saved_p_route(L, name, p):
    io, keep = _case(name, p, backward=True)
    bufs = Bufs()
    f = run_fwd(L, io, bufs, save=True)
    o = run_bwd_stages(L, io, f, bufs, saved=True)
    rep = CK.Report(f"{name} p={p} kernel")
    CK.check_prep(io, f, o.Dv, o.PKX, o.PQX, rep)
    CK.check_saved_route(io, f, o, rep)
    rep.exact("unvisited tiles of dS / dS^T keep the sentinel", corner_sentinel(io, o.dS) and corner_sentinel(io, o.dST))
    rep.exact("guards intact", bufs.guards_intact())
    rep.exact("every dqkv / dpos / Dv element written", bool(torch.isfinite(o.dqkv).all()) and bool(torch.isfinite(o.dpos).all())
              and bool(torch.isfinite(o.Dv).all()))
    end_to_end(io, keep, o, rep)
    prod = run_production(io, f, saved=True)
    rep.exact("disent_attn_bwd: same dS / dS^T", same_corner(io, prod.dS, o.dS) and same_corner(io, prod.dST, o.dST))
    rep.exact("disent_attn_bwd: same dqkv", torch.equal(prod.dqkv, o.dqkv))
    rep.exact("disent_attn_bwd: same dpqk", torch.equal(prod.dpos, o.dpos))
    yard = CK.Report(f"{name} p={p} yardstick")
    CK.check_saved_route(io, f, AR.emulate_bwd(io, f), yard)
    finish(rep, yard)


# ------------------------------------------------------------------------------------------------ backward, recompute
@pytest.mark.parametrize("name", AC.RECOMPUTE_CASES)
def test_recompute_route(L, name):
    p = 0.1
    io, keep = _case(name, p, backward=True)
    bufs = Bufs()
    f = run_fwd(L, io, bufs, save=False)
    o = run_bwd_stages(L, io, f, bufs, saved=False)
    rep = CK.Report(f"{name} p={p} kernel")
    CK.check_prep(io, f, o.Dv, o.PKX, None, rep, QT=o.QT, PQT=o.PQT)
    CK.check_recompute_route(io, f, o, rep, keep)
    rep.exact("unvisited tiles of dS / dS^T keep the sentinel", corner_sentinel(io, o.dS) and corner_sentinel(io, o.dST))
    rep.exact("guards intact", bufs.guards_intact())
    rep.exact("every dqkv / dpos / Dv element written", bool(torch.isfinite(o.dqkv).all()) and bool(torch.isfinite(o.dpos).all())
              and bool(torch.isfinite(o.Dv).all()))
    end_to_end(io, keep, o, rep)
    prod = run_production(io, f, saved=False)
    H = io.H
    rep.exact("disent_attn_bwd: same dS / dS^T", same_corner(io, prod.dS, o.dS) and same_corner(io, prod.dST, o.dST))
    rep.exact("disent_attn_bwd: same dQ, dV", torch.equal(prod.dqkv[:, :H], o.dqkv[:, :H]) and torch.equal(prod.dqkv[:, 2 * H:], o.dqkv[:, 2 * H:]))
    rep.exact("disent_attn_bwd: same dpqk", torch.equal(prod.dpos, o.dpos))
    if int(AC.delta_ranges_np(io.case)[2].max()) == 1:   # no slot of G2 is summed by atomics: the shear pass is order-independent
        rep.exact("disent_attn_bwd: same dK", torch.equal(prod.dqkv[:, H:2 * H], o.dqkv[:, H:2 * H]))
    yard = CK.Report(f"{name} p={p} yardstick")
    CK.check_recompute_route(io, f, AR.emulate_ds_recompute(io, f, keep, o.Dv), yard, keep, only_dS=True)
    finish(rep, yard)
