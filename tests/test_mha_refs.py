"""The case table (tests/mha_cases.py), the float64 references, judges and fp32 yardstick (tests/mha_refs.py) and the checks
(tests/mha_checks.py) of the fused BERT attention, without a GPU.  This is the proof that tests/test_gpu_mha_elementwise.py
would fail if the kernels of mha.hip were subtly wrong:

  * every case reaches what it claims;
  * (a) the closed-form backward equals float64 autograd of the forward formula to 1e-10, with and without a keep mask;
  * (b) the yardstick -- plain fp32 torch with the kernel's rounding points and its tile-wise online softmax -- passes every
    check at every case with S <= 129, at both dropout rates and on packed rows, and needs no more than C / 4 anywhere;
  * (c) eight wrong variants of the yardstick each fail the check that owns them (WRONG below names it);
  * (d) what the bounds cannot be relied on to catch: truncation in the place of round-to-nearest for the bf16 P and dS
    operands.  A truncated value is within 2^-7 of the exact one, on average 2^-8 -- what the worst-case bound must grant
    honest rounding on every term, all of one sign -- and in a sum of mixed signs the biases cancel like the roundings do.
    A bias inside one rounding is below what a worst-case bound resolves; nothing is asserted about the per-element bounds
    for it, only that the variant is a different computation.  (For the record: at s37, p = 0 the truncated variant uses
    0.96 of the ctx bound and 1.07 of the dQ bound on one element of a 7-key sample, and stays inside dK and dV.)
"""
import numpy as np
import pytest
import torch

from tests import mha_cases as MC
from tests import mha_checks as CK
from tests import mha_refs as MR
from tests.attn_refs import inv_keep, old_close
from tests.dropout_replay import attn_mask

F64 = torch.float64


def _io(name, p, plen=None):
    io = MC.make_inputs(name, "cpu", plen=plen)
    io.p, io.seed = p, MC.SEED
    keep = attn_mask(io.seed, io.B, io.nh, io.S, p) if p > 0 else None
    return io, keep


def _pipeline(io, keep, fwd_kw=None, bwd_kw=None, edit_fwd=None, edit_bwd=None):
    """forward -> D -> backward of the yardstick, with the wrong variant's switches / edits, and the full checks on it"""
    f = MR.emulate_fwd(io, keep, **(fwd_kw or {}))
    if edit_fwd:
        edit_fwd(f)
    D = MR.emulate_rowdot(io, f.ctx4)
    o = MR.emulate_bwd(io, keep, f.lse, D, **(bwd_kw or {}))
    if edit_bwd:
        edit_bwd(o)
    rep = CK.Report(f"{io.name} p={io.p} yardstick")
    CK.check_forward(io, keep, f.ctx4, f.lse, rep)
    ctx2d = MR.merge_heads(f.ctx4, io)
    CK.check_backward(io, keep, f.lse, ctx2d, D, o.dQ4, o.dK4, o.dV4, rep)
    CK.check_end_to_end(io, keep, o.dQ4, o.dK4, o.dV4, rep)
    return rep, f, o


def within_quarter(rep):
    """the yardstick's "needs C" of every form: lse in units of C_M (C_L in proportion), the rest in units of C"""
    return all(v <= (MR.C_M if n == "lse" else MR.C) / 4 for n, v in rep.yard.items())


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_is_complete_and_reaches_what_it_claims():
    assert list(MC.CASES) == ["s1", "s37", "s64", "s65", "s129late", "s266", "s266hot", "s512", "s129strided"]
    shapes = {n: (c.B, c.S, c.nh) for n, c in MC.CASES.items()}
    assert shapes == {"s1": (2, 1, 2), "s37": (4, 37, 3), "s64": (3, 64, 2), "s65": (3, 65, 2), "s129late": (4, 129, 3),
                      "s266": (4, 266, 3), "s266hot": (2, 266, 2), "s512": (2, 512, 2), "s129strided": (2, 129, 12)}
    m = {n: c.masks(c.S) for n, c in MC.CASES.items()}
    kl = {n: MC.klen_of(m[n]) for n in m}
    for n in ("s37", "s266"):                        # full; ragged with zeros at keys 1..3; no valid key; short
        S = MC.CASES[n].S
        assert kl[n] == [S, (2 * S) // 3, 0, S // 5] and m[n][1, 1:4].sum() == 0 and m[n][1, 0] == 1 and m[n][1, 4] == 1
    assert kl["s1"] == [1, 0] and kl["s64"] == [64, 63, 1] and kl["s65"] == [65, 64, 0] and kl["s512"] == [512, 341]
    late = m["s129late"]
    assert late[1, :70].sum() == 0 and late[1, 70:].all()                  # the first key tile wholly masked, valid keys after it
    assert late[2, 64] == 1 and late[2, 61:64].sum() == 0 and late[2, 65:68].sum() == 0 and late[2, 60] == 1 and late[2, 68] == 1
    assert MC.key_tiles(kl["s65"][0], 65) == 2 and MC.key_tiles(kl["s65"][1], 65) == 1 and MC.key_tiles(0, 65) == 2
    assert MC.key_tiles(kl["s266"][3], 266) == 1 < MC.key_tiles(kl["s266"][0], 266) == 5 and MC.key_tiles(512, 512) == 8
    c = MC.CASES["s266"]
    assert c.nh % 2 == 1 and not MC.xcd_mapping(c) and kl["s266"] != sorted(kl["s266"], reverse=True)   # border reorders
    assert MC.xcd_mapping(MC.CASES["s129strided"])
    assert MC.CASES["s266hot"].qk_scale == 3.0
    ld, H = MC.STRIDES, 768
    assert len(set(ld.values())) == 8 and not set(ld.values()) & {H, 3 * H} and all(v > H for v in ld.values())
    assert MC.STRIDE_O_ROWS % 8 == 0 and MC.STRIDE_O_ROWS not in set(ld.values()) | {H, 3 * H}
    assert all(ld[n] % 8 == 0 for n in ("q", "k", "v", "dO")) and all(ld[n] % 4 == 0 for n in ("ctx", "dQ", "dK", "dV"))
    assert all(ld[n] % 8 != 0 for n in ("ctx", "dQ", "dK", "dV"))         # the weakest alignment the entry points accept
    for n, plen in MC.ROWS_CASES.items():
        assert any(p > k > 0 for p, k in zip(plen, kl[n])) and any(k == 0 and p == MC.CASES[n].S for p, k in zip(plen, kl[n]))
    io = MC.make_inputs("s129strided")
    assert [getattr(io, n).stride(0) for n in ("q", "k", "v", "dO")] == [ld[n] for n in ("q", "k", "v", "dO")]
    assert torch.equal(io.q, io.fused.q) and torch.equal(io.dO, io.fused.dO) and MC.input_guards_intact(io)
    hot, cold = MC.make_inputs("s266hot"), MC.make_inputs("s266")
    assert hot.q.float().std() > 2.5 * cold.q.float().std() and abs(hot.v.float().std() - cold.v.float().std()) < 0.05


def test_hot_case_moves_the_running_maximum_between_tiles():
    """s266hot: on most rows the maximum is not in the first key tile, so alpha < 1 rescales really happen (and are large)"""
    io, _ = _io("s266hot", 0.0)
    x = MR.widen(io)
    s = MR.reference(x, backward=False).s
    first = s[..., :64].amax(-1)
    assert ((s.amax(-1) - first) > 1.0).double().mean() > 0.5
    assert MR.reference(x, backward=False).P.amax(-1).median() > 0.3       # peaked


# ------------------------------------------------------------------------------------------------ (a) closed form == autograd
@pytest.mark.parametrize("p", MC.P_DROPS)
@pytest.mark.parametrize("name", ["s1", "s37", "s65"])
def test_closed_form_equals_autograd(name, p):
    io, keep = _io(name, p)
    x = MR.widen(io, keep)
    r = MR.reference(x)
    ctx, (gq, gk, gv) = MR.autograd_reference(x)
    scale = max(t.abs().max().item() for t in (gq, gk, gv))
    for nm, a, b in (("ctx", r.ctx, ctx), ("dQ", r.dQ, gq), ("dK", r.dK, gk), ("dV", r.dV, gv)):
        err = (a - b).abs().max().item()
        assert err <= 1e-10 * max(b.abs().max().item(), scale), (nm, err)
    assert torch.isfinite(r.lse).all() and torch.isfinite(r.dS).all()
    # a sample without a valid key: the -10000 is a common offset
    b = [i for i, k in enumerate(io.kl) if k == 0][0]
    assert (r.lse[b] < -9990).all() and (r.lse[b] > -10010).all()
    # masked keys of the other samples: exactly 0 in float64 (exp(-10000) underflows)
    mk = MR.masked_keys(x)[:, None, :, None]
    if bool(mk.any()):
        assert (r.dK[mk.expand_as(r.dK)] == 0).all() and (r.dV[mk.expand_as(r.dV)] == 0).all()


def test_replayed_keep_mask_carries_the_kernels_scale():
    """the non-zero value of the replayed mask is attn_common.h's exact 1 / (1 - p_q) of the 16-bit quantised rate"""
    _, keep = _io("s37", 0.1)
    assert set(keep.unique().tolist()) == {0.0, float(np.float32(inv_keep(0.1)))}
    assert 0.85 < (keep > 0).float().mean().item() < 0.95


def test_end_to_end_bound_is_the_suites_own_in_every_case():
    """dV = keep dO never vanishes, so max|grad| means something even at s1, where dQ = dK = 0 in the reference"""
    for name in MC.CPU_CASES:
        for p in MC.P_DROPS:
            io, keep = _io(name, p)
            refs, atol, floor = CK.end_to_end_atol(io, keep)
            assert not floor and atol == 2e-2 * max(t.abs().max().item() for t in refs) > 0, (name, p)
    io, keep = _io("s1", 0.0)
    dQ, dK, _ = CK.end_to_end_atol(io, keep)[0]
    assert dQ.abs().max() < 1e-12 and dK.abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------ (b) honest roundings pass
@pytest.mark.parametrize("p", MC.P_DROPS)
@pytest.mark.parametrize("name", MC.CPU_CASES)
def test_yardstick_passes_every_check(name, p):
    io, keep = _io(name, p)
    rep, f, o = _pipeline(io, keep)
    print("\n".join(rep.lines()))
    assert rep.failed() == []
    assert within_quarter(rep), rep.yard


@pytest.mark.parametrize("p", MC.P_DROPS)
def test_yardstick_passes_every_check_on_packed_rows(p):
    io, keep = _io("s37", p, plen=MC.ROWS_CASES["s37"])
    rep, f, o = _pipeline(io, keep)
    print("\n".join(rep.lines()))
    assert rep.failed() == []
    assert within_quarter(rep), rep.yard


def test_lse_bound_of_a_sample_without_a_valid_key():
    """where the suite's allclose admits |err| <= 10 the form gives about 1e-2: an error of 0.02 cannot pass"""
    io, keep = _io("s37", 0.0)
    x = MR.widen(io)
    r = MR.reference(x, backward=False)
    bound = MR.U * (MR.C_L + MR.C_M * (r.lse.abs() + r.s.abs().amax(-1)))
    assert 5e-3 < bound[2].min() and bound[2].max() < 1.2e-2
    assert bound[0].max() < 2e-5                                   # an ordinary row: two orders below the 1e-3 of before


# ------------------------------------------------------------------------------------------------ (c) wrong variants fail
def _lse_off(f):
    f.lse[2] += 0.02


def _dk_garbage(io):
    def edit(o):
        mk = MR.masked_keys(MR.widen(io))[:, None, :, None]
        o.dK4[mk.expand_as(o.dK4)] = 1e-3
    return edit


# variant -> (case, p, the check that owns it)
WRONG = {
    "lse_of_the_no_valid_key_sample_off_by_0.02": ("s37", 0.0, "lse"),
    "1e-3_in_dK_at_masked_keys": ("s37", 0.0, "dK = +-0 at masked keys"),
    "one_key_per_tile_left_out_of_dQ": ("s129late", 0.0, "dQ"),
    "last_query_tile_left_out_of_dK": ("s129late", 0.0, "dK"),
    "keep_not_scaled_in_the_backward": ("s37", 0.1, "dQ"),
    "interior_mask_zero_ignored": ("s37", 0.0, "ctx"),
    "alpha_rescale_omitted": ("s129late", 0.0, "ctx"),
    "exp_biased_by_2e-3": ("s65", 0.0, "lse"),
}


@pytest.mark.parametrize("kind", list(WRONG))
def test_wrong_variants_fail_the_check_that_owns_them(kind):
    name, p, owner = WRONG[kind]
    io, keep = _io(name, p)
    kw = dict(fwd_kw=None, bwd_kw=None, edit_fwd=None, edit_bwd=None)
    if kind.startswith("lse_of"):
        kw["edit_fwd"] = _lse_off
    elif kind.startswith("1e-3"):
        kw["edit_bwd"] = _dk_garbage(io)
    elif kind.startswith("one_key"):
        kw["bwd_kw"] = dict(dq_skips_a_key=True)
    elif kind.startswith("last_query"):
        kw["bwd_kw"] = dict(dk_skips_last_tile=True)
    elif kind.startswith("keep_not"):
        kw["bwd_kw"] = dict(keep_unscaled=True)
    elif kind.startswith("interior"):
        kw["fwd_kw"] = dict(ignore_mask=(1, 2))
    elif kind.startswith("alpha"):
        kw["fwd_kw"] = dict(no_alpha=True)
    elif kind.startswith("exp_biased"):
        kw["fwd_kw"] = dict(exp_bias=2e-3)
    rep, f, o = _pipeline(io, keep, **kw)
    print("\n".join(rep.lines()))
    print(f"{kind}: failed {rep.failed()}")
    assert owner in rep.failed(), (kind, rep.failed())
    if kind.startswith("lse_of") or kind.startswith("1e-3"):
        # ... which the tolerances of tests/test_gpu_mha.py let through: lse rtol 1e-3 / atol 1e-3, gradients rtol 3e-2 / atol 2e-2 max
        r = MR.reference(MR.widen(io, keep))
        assert old_close(f.lse, r.lse, 1e-3, 1e-3)
        sc = max(t.abs().max().item() for t in (r.dQ, r.dK, r.dV))
        assert all(old_close(g, t, 3e-2, 2e-2 * sc) for g, t in ((o.dQ4, r.dQ), (o.dK4, r.dK), (o.dV4, r.dV)))


def test_alpha_rescale_also_caught_on_the_hot_case_forward():
    """the same omission where m_run moves between tiles (s266hot), forward only"""
    io, keep = _io("s266hot", 0.0)
    f = MR.emulate_fwd(io, keep, no_alpha=True)
    rep = CK.Report("s266hot, no alpha")
    CK.check_forward(io, keep, f.ctx4, f.lse, rep)
    assert {"lse", "ctx"} <= set(rep.failed())


# ------------------------------------------------------------------------------------------------ (d) below the bounds
def test_truncated_operands_are_a_different_computation():
    """Truncation of the bf16 P and dS operands: see (d) of the module docstring.  Nothing is asserted about the per-element
    bounds -- a bias inside one rounding is below what a worst-case bound resolves -- only that the switch does something."""
    io, keep = _io("s37", 0.0)
    f = MR.emulate_fwd(io, keep)
    ft = MR.emulate_fwd(io, keep, trunc=True)
    D = MR.emulate_rowdot(io, f.ctx4)
    o = MR.emulate_bwd(io, keep, f.lse, D)
    ot = MR.emulate_bwd(io, keep, f.lse, D, trunc=True)
    assert not torch.equal(f.ctx4, ft.ctx4) and torch.equal(f.lse, ft.lse)
    assert not torch.equal(o.dQ4, ot.dQ4) and not torch.equal(o.dV4, ot.dV4)
    rep = CK.Report("s37 truncated operands")
    CK.check_forward(io, keep, ft.ctx4, ft.lse, rep)
    CK.check_backward(io, keep, f.lse, MR.merge_heads(f.ctx4, io), D, ot.dQ4, ot.dK4, ot.dV4, rep)
    print("\n".join(rep.lines()))
