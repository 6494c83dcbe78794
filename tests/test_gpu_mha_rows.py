"""GPU: the packed-row attention of the BERT variant (fbl_mha_fwd_rows / fbl_mha_bwd_rows, include/fbl_mha.h).  The rows that
exist must carry exactly the bits of the padded call on the same data (torch.equal), rows a sample does not have are neither
read nor written, and both agree with the fp32 reference of tests/test_gpu_mha.py at that file's bounds."""
import pytest
import torch

from tests.gpu_refs import heads, stats, unheads
from tests.test_gpu_mha import SCALE, _ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64
NAN = float("nan")

# (B, S, nh, klen, plen)
CASES = [
    (4, 37, 12, [37, 24, 0, 7], [37, 30, 37, 7]),        # plen > klen; a sample with no valid key (keeps all S rows)
    (4, 64, 12, [64, 1, 63, 33], [64, 1, 63, 33]),       # one-row sample; plen at a tile edge and one row short of it
    (4, 129, 12, [129, 64, 65, 1], [129, 64, 65, 1]),    # sample 1 also has zeros at mask positions 1..3
    (4, 266, 16, [266, 177, 0, 53], [266, 200, 266, 64]),
    (3, 512, 12, [512, 341, 102], [512, 341, 128]),
]
IDS = [f"S{c[1]}" for c in CASES]
DROP_SEED = 0x1234567890AB


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


def close(got, ref, rtol, atol, name=""):
    assert torch.allclose(got.float(), ref.float(), rtol=rtol, atol=atol), stats(name, got.float(), ref.float())


_DATA = {}


def _data(case):
    """inputs of one case, built once: the padded grid (arbitrary finite data in every row, as test_gpu_mha._inputs draws it)
    and the packed buffers holding the rows that exist, no slack between samples, plus NaN guard rows"""
    key = CASES.index(case)
    if key in _DATA:
        return _DATA[key]
    B, S, nh, klen, plen = case
    H = nh * 64
    g = torch.Generator().manual_seed(1000 + S + nh)
    qkv = (torch.randn(B * S, 3 * H, generator=g) * 0.7).to(BF16).to(DEV)
    mask = torch.zeros(B, S, dtype=torch.int32)
    for b in range(B):
        mask[b, : klen[b]] = 1
    if S == 129:
        mask[1, 1:4] = 0
    mask = mask.to(DEV)
    sel = torch.cat([b * S + torch.arange(plen[b]) for b in range(B)]).to(DEV)
    Np = sel.numel()
    row0 = torch.tensor([sum(plen[:b]) for b in range(B + 1)], dtype=torch.int32, device=DEV)
    kl = torch.tensor(klen, dtype=torch.int32, device=DEV)
    qkv_p = torch.full((Np + GUARD, 3 * H), NAN, dtype=BF16, device=DEV)
    qkv_p[:Np] = qkv[sel]
    dO_p = torch.full((Np + GUARD, H), NAN, dtype=BF16, device=DEV)
    dO_p[:Np] = torch.randn(Np, H, generator=g).to(BF16).to(DEV)
    dO = torch.zeros(B * S, H, dtype=BF16, device=DEV)  # the padded comparison run: the same dO scattered, zeros elsewhere
    dO[sel] = dO_p[:Np]
    d = dict(B=B, S=S, nh=nh, H=H, plen=plen, qkv=qkv, mask=mask, sel=sel, Np=Np, row0=row0, klen=kl, qkv_p=qkv_p, dO_p=dO_p, dO=dO,
             border=torch.argsort(kl, descending=True, stable=True).to(torch.int32), pad={}, ref={})
    _DATA[key] = d
    return d


def _padded(L, d, p_drop):
    """lib.mha_fwd / attn_rowdot / lib.mha_bwd on the padded grid, once per (case, p_drop)"""
    if p_drop in d["pad"]:
        return d["pad"][p_drop]
    B, S, nh, H, qkv = d["B"], d["S"], d["nh"], d["H"], d["qkv"]
    kw = dict(p_drop=p_drop, seed=DROP_SEED if p_drop else 0, klen=d["klen"], border=d["border"])
    ctx = torch.empty(B * S, H, dtype=BF16, device=DEV)
    lse = torch.empty(B, nh, S, device=DEV)
    L.mha_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], d["mask"].view(-1), SCALE, ctx, lse, B, S, nh, **kw)
    Dv = torch.empty(B, nh, S, device=DEV)
    L.attn_rowdot(d["dO"], ctx, Dv, B, S, nh)
    dqkv = torch.empty(B * S, 3 * H, dtype=BF16, device=DEV)
    L.mha_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], d["dO"], d["mask"].view(-1), lse, Dv, SCALE, dqkv[:, :H],
              dqkv[:, H:2 * H], dqkv[:, 2 * H:], B, S, nh, **kw)
    d["pad"][p_drop] = (ctx, lse, dqkv)
    return d["pad"][p_drop]


def _fwd_rows(L, d, p_drop=0.0):
    B, S, nh, H, q = d["B"], d["S"], d["nh"], d["H"], d["qkv_p"]
    ctx = torch.full((d["Np"] + GUARD, H), NAN, dtype=BF16, device=DEV)
    lse = torch.full((B, nh, S), NAN, device=DEV)
    L.mha_fwd_rows(q[:, :H], q[:, H:2 * H], q[:, 2 * H:], d["mask"].view(-1), d["klen"], d["row0"], SCALE, ctx, lse, B, S, nh,
                   p_drop=p_drop, seed=DROP_SEED if p_drop else 0, border=d["border"])
    return ctx, lse


def _bwd_rows(L, d, ctx, lse, p_drop=0.0):
    B, S, nh, H, q = d["B"], d["S"], d["nh"], d["H"], d["qkv_p"]
    dqkv = torch.full((d["Np"] + GUARD, 3 * H), NAN, dtype=BF16, device=DEV)
    Dv = torch.full((B, nh, S), NAN, device=DEV)
    L.mha_bwd_rows(q[:, :H], q[:, H:2 * H], q[:, 2 * H:], d["dO_p"], ctx, d["mask"].view(-1), d["klen"], d["row0"], lse, Dv, SCALE,
                   dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:], B, S, nh, p_drop=p_drop, seed=DROP_SEED if p_drop else 0,
                   border=d["border"])
    return dqkv, Dv


def _lse_rows_equal(d, lse_p, lse):
    """lse at the positions that have a row equals the padded call's; the others were not written"""
    for b, pl in enumerate(d["plen"]):
        assert torch.equal(lse_p[b, :, :pl], lse[b, :, :pl]), f"lse of sample {b}"
        assert bool(torch.isnan(lse_p[b, :, pl:]).all()), f"lse of sample {b} written beyond plen"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mha_fwd_rows(L, case):
    d = _data(case)
    B, S, nh, Np, sel = d["B"], d["S"], d["nh"], d["Np"], d["sel"]
    ctx, lse, _ = _padded(L, d, 0.0)
    ctx_p, lse_p = _fwd_rows(L, d)
    assert not bool(torch.isnan(ctx_p[:Np]).any())        # every existing row written, none of it from a guard row
    assert bool(torch.isnan(ctx_p[Np:]).all())            # the guard rows are untouched
    assert torch.equal(ctx_p[:Np], ctx[sel])
    _lse_rows_equal(d, lse_p, lse)
    # ... and the fp32 reference on the padded grid
    ref, rlse = _ref(d["qkv"].float(), d["mask"], B, S, nh)
    close(ctx_p[:Np], unheads(ref)[sel], 2e-2, 2e-2, f"ctx S={S}")
    for b, pl in enumerate(d["plen"]):
        close(lse_p[b, :, :pl], rlse[b, :, :pl], 1e-3, 1e-3, "lse")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mha_bwd_rows(L, case):
    d = _data(case)
    B, S, nh, H, Np, sel = d["B"], d["S"], d["nh"], d["H"], d["Np"], d["sel"]
    _, _, dqkv = _padded(L, d, 0.0)
    ctx_p, lse_p = _fwd_rows(L, d)
    dq_p, Dv = _bwd_rows(L, d, ctx_p, lse_p)
    assert not bool(torch.isnan(dq_p[:Np]).any())
    assert bool(torch.isnan(dq_p[Np:]).all())             # the guard rows are untouched
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)), ("dV", slice(2 * H, 3 * H))):
        assert torch.equal(dq_p[:Np, sl], dqkv[sel][:, sl]), name
    for b, pl in enumerate(d["plen"]):                    # D is formed for the rows that exist, nothing beyond
        assert not bool(torch.isnan(Dv[b, :, :pl]).any()) and bool(torch.isnan(Dv[b, :, pl:]).all())
    # autograd through the fp32 reference (dO is zero at the rows that do not exist)
    qf = d["qkv"].float().requires_grad_(True)
    ref, _ = _ref(qf, d["mask"], B, S, nh)
    (unheads(ref) * d["dO"].float()).sum().backward()
    sc = qf.grad.abs().max().item()
    for name, sl in (("dQ", slice(0, H)), ("dK", slice(H, 2 * H)), ("dV", slice(2 * H, 3 * H))):
        close(dq_p[:Np, sl], qf.grad[sel][:, sl], 3e-2, 2e-2 * sc, f"{name} S={S}")
    # no atomics: two calls give identical bits
    again, _ = _bwd_rows(L, d, ctx_p, lse_p)
    assert torch.equal(again[:Np], dq_p[:Np])


@pytest.mark.parametrize("case", [CASES[2], CASES[3]], ids=[IDS[2], IDS[3]])
def test_mha_rows_dropout_draws_the_padded_calls_decisions(L, case):
    d = _data(case)
    H, Np, sel = d["H"], d["Np"], d["sel"]
    ctx, lse, dqkv = _padded(L, d, 0.1)
    ctx_p, lse_p = _fwd_rows(L, d, 0.1)
    assert torch.equal(ctx_p[:Np], ctx[sel])
    _lse_rows_equal(d, lse_p, lse)
    dq_p, _ = _bwd_rows(L, d, ctx_p, lse_p, 0.1)
    assert torch.equal(dq_p[:Np], dqkv[sel])
    assert bool(torch.isnan(dq_p[Np:]).all()) and bool(torch.isnan(ctx_p[Np:]).all())
    ctx0, _ = _fwd_rows(L, d)
    assert (ctx0[:Np].float() - ctx_p[:Np].float()).abs().max().item() > 1e-2  # dropout did something
