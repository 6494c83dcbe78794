"""The attention case table (tests/attn_cases.py) and the float64 references / judges (tests/attn_refs.py, with the checks
of tests/attn_checks.py), without a GPU.

  * every case reaches what it claims -- proved from the host formulas (rel_index_vector, the delta ranges, the `band` condition
    of attn_fwd.hip, wg_coord's (nh * B) & 7);
  * (a) the closed-form backward equals float64 autograd of the forward formula to 1e-10, with and without a keep mask;
  * (b) a torch emulation of the kernels' documented rounding points (fp16 bias tiles, tile-wise online softmax, bf16 psave,
    fp32 elsewhere: attn_refs.emulate_fwd / emulate_bwd) passes every judge: the reference plus honest rounding stays inside
    the forms;
  * (c) six wrong results each fail the judge that owns them.  OLD says what the global tolerances the suite had before
    (ctx 2e-2 / 2e-2, lse 1e-3 / 1e-3, gradients rtol 3e-2 + atol 2e-2 max|ref|) make of the same wrong result.
"""
import numpy as np
import pytest
import torch

from tests import attn_cases as AC
from tests import attn_checks as CK
from tests import attn_refs as AR
from tests.dropout_replay import attn_mask


def _io(name, p, backward):
    io = AC.make_inputs(name, "cpu", backward=backward)
    io.p, io.seed = p, AC.SEED
    keep = attn_mask(io.seed, io.B, io.nh, io.S, p) if p > 0 else None
    return io, keep


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_is_complete_and_well_formed():
    assert list(AC.CASES) == ["s1", "s37", "s64", "s130", "s266x", "s266p", "s512", "coarse", "clamped"]
    assert set(AC.RECOMPUTE_CASES) <= set(AC.CASES)
    for name, c in AC.CASES.items():
        assert 1 <= c.S <= 512 and AC.pad64(c.S) % 64 == 0, name          # attn_common.h grid_shape_ok
        assert 2 * AC.lin_fwd(c) <= AC.span2_of(c), name                    # fbl_disent_attn_fwd's argument check
        rv = AC.relidx_np(c)
        assert rv.shape == (2 * c.S - 1,) and (np.diff(rv) >= 0).all() and (np.diff(rv) <= 1).all(), name   # monotone, slope <= 1
        assert 0 <= rv.min() and rv.max() < AC.span2_of(c), name
        m = AC.mask_np(c)
        kl, lens = AC.lengths(c)
        assert all(m[b, kl[b]:].sum() == 0 for b in range(c.B)), name      # nothing valid beyond klen
        if c.packed:
            assert c.klen is not None and lens == kl                         # the packed layout is defined by the lengths


def _tile_pairs(c):
    for b in range(c.B):
        nq, nk = AC.visited_tiles(c, b)
        for it in range(nq):
            for jt in range(nk):
                yield b, it * 64, jt * 64


def test_every_case_reaches_what_it_claims():
    C = AC.CASES
    c = C["s1"]
    assert c.S == 1 and AC.pad64(1) == 64 and c.klen is None                # the smallest grid the entry points accept
    c = C["s37"]
    assert AC.pad64(c.S) == 64 > c.S and all(AC.band(i0, j0, AC.lin_fwd(c)) for _, i0, j0 in _tile_pairs(c))
    m = AC.mask_np(c)
    assert m[0, -1] == 0 and m[0, 0] == 1 and m[1, 1] == 0 and m[1, 0] == 1 and m[1, -1] == 1   # a tail and interior keys
    c = C["s64"]
    assert c.S == AC.pad64(c.S) == 64 and c.B * c.nh == 1
    c = C["s130"]
    pairs = list(_tile_pairs(c))
    assert any(not AC.band(i0, j0, AC.lin_fwd(c)) for _, i0, j0 in pairs)
    assert all(AC.band(i0, j0, AC.lin_fwd(c)) == (abs(i0 - j0) < 128) for _, i0, j0 in pairs)  # only tile distance 2 is outside
    # the first log buckets: deltas +-128, +-129 are beyond position_buckets / 2 (the map's log branch; its first buckets still
    # hold one delta each, so the kernels' `lin` is what separates them from the band, not the values)
    assert c.S - 1 >= c.cmap[0] // 2 == AC.lin_fwd(c) and AC.delta_ranges_np(c)[2].max() == 1
    assert AC.mask_np(c)[0, -1] == 0
    c = C["s266x"]
    assert AC.xcd_mapping(c) and not AC.xcd_mapping(C["s130"])
    assert c.border and list(c.klen) != sorted(c.klen, reverse=True)           # the dispatch order is not the sample order
    assert min(AC.visited_tiles(c, b)[0] for b in range(c.B)) < AC.pad64(c.S) // 64   # query tiles beyond klen
    assert AC.delta_ranges_np(c)[2].max() == 3
    c = C["s266p"]
    assert c.packed and sum(AC.lengths(c)[1]) < c.B * c.S                    # rows without their padding: row0 is not b * S
    assert sorted(c.klen) == sorted(C["s266x"].klen) and not c.border        # the same lengths, sample order = dispatch order
    c = C["s512"]
    assert c.S == AC.pad64(c.S) == 512 and AC.delta_ranges_np(c)[2].max() == 6
    rv = AC.relidx_np(c).astype(int)
    span2 = AC.span2_of(c)
    r_lo = [rv[i0 - (j0 + 63) + c.S - 1] for _, i0, j0 in _tile_pairs(c) if not AC.band(i0, j0, AC.lin_fwd(c))]
    assert max(r_lo) + 127 > span2 - 1                                       # the window's row loads are clamped at the table's end
    c = C["coarse"]
    assert AC.lin_fwd(c) == 32 and not any(AC.band(i0, j0, 32) for _, i0, j0 in _tile_pairs(c))
    assert AC.delta_ranges_np(c)[2].max() > 8                                # fbl_attn_pos_grad: the prefix-difference kernel
    c = C["clamped"]
    assert AC.lin_fwd(c) == 0 and AC.lin_bwd(c) == (0, c.cmap[2] - 1)
    _, dlo, dcnt = AC.delta_ranges_np(c)
    assert dcnt[0] > 8 and dcnt[-1] > 8 and (dcnt[1:-1] == 1).all()          # every delta beyond the span on the two edge rows


# ------------------------------------------------------------------------------------------------ (a) closed form == autograd
@pytest.mark.parametrize("p", AC.P_DROPS)
@pytest.mark.parametrize("name", ["s37", "s130", "coarse"])
def test_closed_form_equals_autograd(name, p):
    io, keep = _io(name, p, backward=True)
    x = AR.widen(io, keep)
    r = AR.reference(x)
    ctx, (gq, gk, gv, gpk, gpq) = AR.autograd_reference(x)
    live = x.valid[:, None, :, None]
    for nm, a, b in (("ctx", r.ctx, ctx), ("dQ", r.dQ, gq), ("dK", r.dK, gk), ("dV", r.dV, gv), ("dPK", r.dPK, gpk), ("dPQ", r.dPQ, gpq)):
        if a.shape == ctx.shape:
            a, b = a * live, b * live
        err = (a - b).abs().max().item()
        assert err <= 1e-10 * b.abs().max().item(), (nm, err)
    assert r.dS.abs().max() > 0 and torch.isfinite(r.dS).all()


# ------------------------------------------------------------------------------------------------ (b) honest roundings pass
_EMU = {}


def _emulated(name, p, backward):
    key = (name, p, backward)
    if key not in _EMU:
        io, keep = _io(name, p, backward)
        f = AR.emulate_fwd(io, keep)
        o = AR.emulate_bwd(io, f) if backward else None
        _EMU[key] = (io, keep, f, o)
    return _EMU[key]


def _judge_all(io, keep, f, o):
    rep = CK.Report(io.name)
    CK.check_forward(io, f, keep, rep)
    if o is not None:
        CK.check_prep(io, f, o.Dv, None, None, rep)
        CK.check_saved_route(io, f, o, rep)
    return rep


@pytest.mark.parametrize("backward", [False, True], ids=["fwd_inputs", "bwd_inputs"])
@pytest.mark.parametrize("p", AC.P_DROPS)
@pytest.mark.parametrize("name", ["s130", "s266x"])
def test_honest_roundings_pass_every_judge(name, p, backward):
    io, keep, f, o = _emulated(name, p, backward)
    rep = _judge_all(io, keep, f, o)
    print("\n".join(rep.lines()))
    assert rep.failed() == []
    # the yardstick of the measured constants stays within C / 4
    assert rep.yard["P"] <= AR.C_P / 4 and rep.yard["lse"] <= AR.C_LSE / 4
    assert _old_forward_pass(io, keep, f)   # (what the old tolerances are measured against in (c))
    if o is not None:
        assert rep.yard["dS"] <= AR.C_DS / 4
        # ... and the emulated pipeline is a sane backward: the old global tolerance holds against the full reference
        assert _old_gradients_pass(io, keep, o)


def _old_forward_pass(io, keep, f):
    x = AR.widen(io, keep)
    r = AR.reference(x, backward=False)
    qv = x.valid[:, None, :].expand_as(r.lse)
    ctx = AR.split_heads(f.ctx, io)
    return (AR.old_close(ctx, r.ctx, 2e-2, 2e-2) and AR.old_close(f.lse[qv], r.lse[qv], 1e-3, 1e-3)
            and bool(torch.isinf(f.lse[~qv]).all()))


def _old_gradients_pass(io, keep, o):
    """test_gpu_kernels.py::test_attention_bwd's bound, plain: rtol 3e-2, atol 2e-2 max|ref| over dqkv resp. dpqk"""
    x = AR.widen(io, keep)
    r = AR.reference(x)
    H = io.H
    ref = torch.cat([AR.merge_heads(t, io) for t in (r.dQ, r.dK, r.dV)], 1)
    rpos = torch.cat([r.dPQ.permute(1, 0, 2).reshape(-1, H), r.dPK.permute(1, 0, 2).reshape(-1, H)], 1)
    return (AR.old_close(o.dqkv, ref, 3e-2, 2e-2 * ref.abs().max().item())
            and AR.old_close(o.dpqk, rpos, 3e-2, 2e-2 * rpos.abs().max().item()))


def test_end_to_end_bound_is_the_suites_own_wherever_the_reference_does_not_vanish():
    """the end-to-end atol is the suite's 2e-2 max|ref|, unmodified, for every tensor of every case -- but dpqk of s1, whose reference
    is identically zero (one key: dS = 0) and which alone gets the rounding floor of attn_checks.end_to_end_atols"""
    for name in AC.CASES:
        for p in AC.P_DROPS:
            io, keep = _io(name, p, backward=True)
            ref, rpos, a0, a1, vanishes = CK.end_to_end_atols(io, keep)
            assert vanishes == (False, name == "s1"), (name, p, vanishes)
            assert a0 == 2e-2 * ref.abs().max().item() > 0
            if name == "s1":
                assert rpos.abs().max().item() < 1e-12 < a1
            else:
                assert a1 == 2e-2 * rpos.abs().max().item() > 0


# ------------------------------------------------------------------------------------------------ (c) wrong results fail
# perturbation -> (the check that owns it, whether the old global tolerance ALSO catches it)
OLD = {
    "neighbouring_table_row": ("P", False),
    "dropout_block_flipped": ("psave sign bit = replayed drop decision", True),
    "last_key_left_out": ("P", True),
    "D_from_undropped_P": ("D", True),
    "keep_scale_missing": ("dS", True),
    "dST_tile_not_transposed": ("dS^T = transpose of dS", True),
}


def _perturbed(kind):
    name, p = "s130", 0.1
    backward = kind in ("D_from_undropped_P", "keep_scale_missing", "dST_tile_not_transposed")
    io, keep = _io(name, p, backward)
    S = io.S
    if kind == "neighbouring_table_row":
        ri = io.relidx.clone()
        d = 128                                      # outside the identity band (|delta| >= 128)
        assert ri[S - 1 + d] != ri[S - 1 + d - 1]
        ri[S - 1 + d] -= 1
        f = AR.emulate_fwd(io, keep, relidx=ri)
    elif kind == "dropout_block_flipped":
        k2 = keep.clone()
        blk = k2[1, 0, 40:42, 70:72]
        inv = keep.max()
        k2[1, 0, 40:42, 70:72] = torch.where(blk == 0, inv, torch.zeros_like(blk))
        f = AR.emulate_fwd(io, k2)
    elif kind == "last_key_left_out":
        f = AR.emulate_fwd(io, keep, drop_key=(1, slice(None), slice(None), io.kl[1] - 1))
    else:
        f = AR.emulate_fwd(io, keep)
    o = None
    if kind == "D_from_undropped_P":
        o = AR.emulate_bwd(io, f, D_from=AR.emulate_fwd(io, None).ctx)
    elif kind == "keep_scale_missing":
        o = AR.emulate_bwd(io, f, p_scaled=False)
    elif kind == "dST_tile_not_transposed":
        o = AR.emulate_bwd(io, f, transpose_tile=(1, 1, 1, 0))
    return io, keep, f, o


@pytest.mark.parametrize("kind", list(OLD))
def test_wrong_results_fail_the_judge_that_owns_them(kind):
    owner, old_catches = OLD[kind]
    io, keep, f, o = _perturbed(kind)
    rep = _judge_all(io, keep, f, o)
    print("\n".join(rep.lines()))
    assert owner in rep.failed(), (kind, rep.failed())
    old_ok = _old_forward_pass(io, keep, f) if o is None else _old_gradients_pass(io, keep, o)
    print(f"{kind}: the old global tolerance {'passes' if old_ok else 'fails'} it")
    assert old_ok == (not old_catches), kind
