"""The fused BERT attention (frozenbilm_amd/csrc/mha.hip: fbl_mha_fwd, fbl_mha_bwd, fbl_mha_fwd_rows, fbl_mha_bwd_rows) on the
MI355X, element by element, against the float64 references of tests/mha_refs.py, at the cases of tests/mha_cases.py, without
and with attention dropout (p = 0.1).  The dropout masks are rebuilt on the host (tests/dropout_replay.attn_mask) and applied
inside the reference.

Per case and p_drop: the outputs are prefilled with sentinels and have guards behind (and, in the strided case, between) their
rows; mha_fwd, attn_rowdot and mha_bwd run as the engine runs them; the forward is judged on the input bits, the backward on
its own input bits (the lse the forward stored, the D that was written).  Every element of every output is judged: the share
left out of the bounded checks is 0 (masked keys have reference 0 and bound 0, which admits only +-0).
tests/test_mha_refs.py is the CPU proof that these checks fail on a subtly wrong kernel.

(a) Exact.  dK = dV = +-0 at every masked key of a sample that has a valid key, the key tiles beyond klen included; lse finite on
    every row; every output element written, guard rows and guard columns intact, inputs untouched; rows beyond a packed
    sample's plen untouched (ctx, dQ, dK, dV have no such rows; lse and D keep their sentinel there); the call with klen and
    border = the call without, bit for bit; the strided call = the fused-buffer call on the same data = the packed entries on the
    same rows (which take dO and ctx with a row stride each and form D themselves), bit for bit; a second run = the first, bit
    for bit (no atomics).

(b) Forms (u = 2^-24; s2 = s log2 e with the mask bias, lse2 = lse log2 e; n = S + Sp / 64).  The constants C = 16, C_L = 64,
    C_M = 8 are counts of the fp32 roundings of mha.hip (tests/mha_refs.py), not fitted to the kernel.  Every run recomputes the
    yardstick -- plain fp32 torch with the same rounding points and the same tile-wise online softmax (mha_refs.emulate_fwd /
    emulate_bwd), never the HIP kernel --, asserts it within C / 4 and the kernel within C.
      lse     u (C_L + C_M (|lse| + max_j |s|))
      ctx     sum_j keep |v| P (2^-8 + C u (1 + |s2| + |lse2|)) + 2 (2 n) u sum|term| + 2^-8 |ctx|
      D       2 64 u sum|dO ctx|                                                       (padded: fbl_attn_rowdot; rows: the rows kernel)
      dV      sum_i keep |dO| P (2^-8 + C u (1 + |s2| + |lse2|)) + 2 n u sum|term| + 2^-8 |dV|          P = exp(s - lse_bits)
      dQ, dK  sum (2^-8 |dS| + 2 64 u P keep sum|dO v| scale + C u P scale (keep |dP| + |D|) (1 + |s2| + |lse2|)) |K| resp. |Q|
              + 2 n u sum|term| + 2^-8 |ref|
    "needs C": the smallest C at which the form holds for every element (lse: the C_M, with C_L in proportion).

    quantity   yardstick needs C   C          kernel needs C   worst |err| / bound: yardstick (at)      kernel (at)
    lse        0.99                8 (64)     0.94             0.124  s266hot p=0         0.117  s266 p=0
    ctx        0.00                16         0.00             0.686  s266hot p=0.1       0.686  s266hot p=0.1
    D          -                   -          -                -                          0.009  s512 p=0
    dV         0.00                16         0.00             0.814  s266hot p=0.1       0.814  s266hot p=0.1
    dQ         0.00                16         0.00             0.852  s266hot p=0.1       0.852  s266hot p=0.1
    dK         0.00                16         0.00             0.801  s266hot p=0.1       0.801  s266hot p=0.1

    (measured on an MI355X, ROCm 7.0 runtime (torch 2.10.0+rocm7.0, HIP 7.0.51831), kernels built by the hipcc of ROCm 7.2;
    all cases and the two packed ones, p = 0 and 0.1.)  Only lse ever reaches its fp32 term:
    its form has no bf16 part, and kernel and yardstick use an eighth of it.  Everywhere else neither leaves the bf16 part of
    the forms (2^-8 per term, three orders above the fp32 part on ordinary rows; on a row without a valid key the two are of
    one size and the errors stay below both), so C = 16 is counted, not measured, and kernel and yardstick agree to the third
    digit.  No constant had to be recounted.

(c) End to end.  dQ, dK, dV against the full float64 reference at the suite's own global tolerance (tests/test_gpu_mha.py: rtol
    3e-2, atol 2e-2 max|grad|; mha_checks.end_to_end_atol for s1, where dQ and dK vanish in the reference).

The packed entries are judged directly at two cases (mha_cases.ROWS_CASES: plen > klen on one sample, the sample without a
valid key keeps all its rows); their bit equality with the padded call stays the job of tests/test_gpu_mha_rows.py.
"""
import types

import pytest
import torch

from tests import mha_cases as MC
from tests import mha_checks as CK
from tests import mha_refs as MR
from tests.attn_refs import SENT_BF16, SENT_F32
from tests.dropout_replay import attn_mask

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
G = 8  # guard elements of the fp32 outputs (the row buffers: MC.GUARD_ROWS rows)


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


class Bufs:
    """sentinel-prefilled outputs with guards behind them and, where the row stride exceeds the width, between the rows"""

    def __init__(self):
        self.rows_, self.flat_ = [], []

    def rows(self, rows, ld, width):
        full = MC.sentinel_rows(rows, ld, DEV)
        self.rows_.append((full, rows, width))
        return full[:rows, :width]

    def flat(self, shape):
        n = 1
        for s in shape:
            n *= s
        full = torch.empty(n + G, dtype=F32, device=DEV)
        full.view(torch.int32).fill_(SENT_F32)
        self.flat_.append((full, n))
        return full[:n].view(*shape)

    def guards_intact(self):
        ok = all(bool((full.view(torch.int32)[n:] == SENT_F32).all()) for full, n in self.flat_)
        for full, rows, width in self.rows_:
            bits = full.view(torch.int16)
            ok &= bool((bits[rows:] == SENT_BF16).all()) and bool((bits[:rows, width:] == SENT_BF16).all())
        return ok


def _case(name, p, plen=None):
    io = MC.make_inputs(name, DEV, plen=plen)
    io.p, io.seed = p, MC.SEED
    keep = attn_mask(io.seed, io.B, io.nh, io.S, p).to(DEV) if p > 0 else None
    return io, keep


def run(L, io, bufs, src=None, hints=True, ld=None):
    """mha_fwd -> attn_rowdot -> mha_bwd (packed: mha_fwd_rows -> mha_bwd_rows) into fresh sentinel-prefilled outputs.
    src: where q, k, v, dO come from (io by default); hints: pass klen and border; ld: the outputs' row strides."""
    src = src or io
    ld = ld or io.ld
    B, S, nh, H, rows = io.B, io.S, io.nh, io.H, io.rows
    o = types.SimpleNamespace()
    o.ctx = bufs.rows(rows, ld["ctx"], H)
    o.lse = bufs.flat((B, nh, S))
    o.Dv = bufs.flat((B, nh, S))
    if ld["dQ"] == 3 * H:                        # dQ | dK | dV fused, as the engine keeps them
        dqkv = bufs.rows(rows, 3 * H, 3 * H)
        o.dQ, o.dK, o.dV = (dqkv[:, i * H:(i + 1) * H] for i in range(3))
    else:
        o.dQ, o.dK, o.dV = (bufs.rows(rows, ld[n], H) for n in ("dQ", "dK", "dV"))
    kw = dict(p_drop=io.p, seed=io.seed if io.p > 0 else 0)
    mask = io.mask.view(-1)
    if io.packed:
        L.mha_fwd_rows(src.q, src.k, src.v, mask, io.klen, io.row0, io.scale, o.ctx, o.lse, B, S, nh, border=io.border, **kw)
        L.mha_bwd_rows(src.q, src.k, src.v, src.dO, o.ctx, mask, io.klen, io.row0, o.lse, o.Dv, io.scale, o.dQ, o.dK, o.dV, B, S, nh,
                       border=io.border, **kw)
    else:
        if hints:
            kw.update(klen=io.klen, border=io.border)
        L.mha_fwd(src.q, src.k, src.v, mask, io.scale, o.ctx, o.lse, B, S, nh, **kw)
        ctx_dot = o.ctx
        if o.ctx.stride(0) != src.dO.stride(0):  # fbl_attn_rowdot takes one row stride for dO and ctx: hand it the same bits
            ctx_dot = bufs.rows(rows, src.dO.stride(0), H)
            ctx_dot.copy_(o.ctx)
        L.attn_rowdot(src.dO, ctx_dot, o.Dv, B, S, nh)
        L.mha_bwd(src.q, src.k, src.v, src.dO, mask, o.lse, o.Dv, io.scale, o.dQ, o.dK, o.dV, B, S, nh, **kw)
    torch.cuda.synchronize()
    return o


def run_rows_strided(L, io, bufs):
    """fbl_mha_fwd_rows / fbl_mha_bwd_rows on the strided case's own buffers, every sample keeping all its rows (row0 = b S).
    fbl_mha_bwd_rows forms D itself and takes dO and the forward's output with a row stride each (the latter a multiple of 8:
    the ctx bits are handed over in a buffer of MC.STRIDE_O_ROWS)."""
    B, S, nh, H, rows, ld = io.B, io.S, io.nh, io.H, io.rows, io.ld
    row0 = (torch.arange(B + 1, dtype=torch.int32) * S).to(DEV)
    o = types.SimpleNamespace()
    o.ctx = bufs.rows(rows, ld["ctx"], H)
    o.lse, o.Dv = bufs.flat((B, nh, S)), bufs.flat((B, nh, S))
    o.dQ, o.dK, o.dV = (bufs.rows(rows, ld[n], H) for n in ("dQ", "dK", "dV"))
    kw = dict(p_drop=io.p, seed=io.seed if io.p > 0 else 0, border=io.border)
    mask = io.mask.view(-1)
    L.mha_fwd_rows(io.q, io.k, io.v, mask, io.klen, row0, io.scale, o.ctx, o.lse, B, S, nh, **kw)
    O = bufs.rows(rows, MC.STRIDE_O_ROWS, H)
    O.copy_(o.ctx)
    L.mha_bwd_rows(io.q, io.k, io.v, io.dO, O, mask, io.klen, row0, o.lse, o.Dv, io.scale, o.dQ, o.dK, o.dV, B, S, nh, **kw)
    torch.cuda.synchronize()
    return o


def same_bits(a, b):
    """(as integers: what a packed call leaves untouched is the NaN sentinel)"""
    iv = {BF16: torch.int16, F32: torch.int32}
    return all(torch.equal(getattr(a, n).contiguous().view(iv[getattr(a, n).dtype]), getattr(b, n).contiguous().view(iv[getattr(b, n).dtype]))
               for n in ("ctx", "lse", "Dv", "dQ", "dK", "dV"))


def judge(io, keep, o, rep):
    h4 = lambda t: MR.split_heads(t, io)
    CK.check_forward(io, keep, h4(o.ctx), o.lse, rep)
    CK.check_backward(io, keep, o.lse, o.ctx, o.Dv, h4(o.dQ), h4(o.dK), h4(o.dV), rep)
    CK.check_end_to_end(io, keep, h4(o.dQ), h4(o.dK), h4(o.dV), rep)


def judge_yardstick(io, keep, o, yard):
    """the yardstick on the same inputs: its forward on the input bits, its backward on the lse and D bits the kernels wrote"""
    f = MR.emulate_fwd(io, keep)
    CK.check_forward(io, keep, f.ctx4, f.lse, yard)
    e = MR.emulate_bwd(io, keep, o.lse, o.Dv)
    CK.check_backward(io, keep, o.lse, o.ctx, o.Dv, e.dQ4, e.dK4, e.dV4, yard)


def finish(rep, yard):
    print("\n".join(rep.lines()))
    print("\n".join(yard.lines()))
    assert yard.failed() == [], yard.failed()
    for n, v in yard.yard.items():
        assert v <= (MR.C_M if n == "lse" else MR.C) / 4, (n, v)
    assert rep.failed() == [], rep.failed()


def written(o):
    return all(bool(torch.isfinite(getattr(o, n)).all()) for n in ("ctx", "dQ", "dK", "dV"))


@pytest.mark.parametrize("p", MC.P_DROPS)
@pytest.mark.parametrize("name", list(MC.CASES))
def test_mha_elementwise(L, name, p):
    io, keep = _case(name, p)
    bufs = Bufs()
    o = run(L, io, bufs)
    rep = CK.Report(f"{name} p={p} kernel")
    judge(io, keep, o, rep)
    rep.exact("every output element written", written(o) and bool(torch.isfinite(o.lse).all()) and bool(torch.isfinite(o.Dv).all()))
    rep.exact("the call without klen and border: same bits", same_bits(o, run(L, io, bufs, hints=False)))
    rep.exact("a second run: same bits", same_bits(o, run(L, io, bufs)))
    if io.strided:
        H = io.H
        fused = run(L, io, bufs, src=io.fused, ld=dict(ctx=H, dQ=3 * H, dK=3 * H, dV=3 * H))
        rep.exact("the fused-buffer call on the same data: same bits", same_bits(o, fused))
        rep.exact("the packed entries on the same rows, dO and ctx with a stride each: same bits", same_bits(o, run_rows_strided(L, io, bufs)))
    rep.exact("guards intact", bufs.guards_intact())
    rep.exact("inputs untouched", MC.input_guards_intact(io))
    yard = CK.Report(f"{name} p={p} yardstick")
    judge_yardstick(io, keep, o, yard)
    finish(rep, yard)


@pytest.mark.parametrize("p", MC.P_DROPS)
@pytest.mark.parametrize("name", list(MC.ROWS_CASES))
def test_mha_rows_elementwise(L, name, p):
    io, keep = _case(name, p, plen=MC.ROWS_CASES[name])
    bufs = Bufs()
    o = run(L, io, bufs)
    rep = CK.Report(f"{name} rows p={p} kernel")
    judge(io, keep, o, rep)
    has = MR.widen(io).hasq.expand_as(o.lse)
    rep.exact("every output element written", written(o) and bool(torch.isfinite(o.lse[has]).all()) and bool(torch.isfinite(o.Dv[has]).all()))
    rep.exact("lse and D untouched beyond plen", bool((o.lse.view(torch.int32)[~has] == SENT_F32).all())
              and bool((o.Dv.view(torch.int32)[~has] == SENT_F32).all()))
    rep.exact("a second run: same bits", same_bits(o, run(L, io, bufs)))
    rep.exact("guards intact", bufs.guards_intact())
    rep.exact("inputs untouched", MC.input_guards_intact(io))
    yard = CK.Report(f"{name} rows p={p} yardstick")
    judge_yardstick(io, keep, o, yard)
    finish(rep, yard)
