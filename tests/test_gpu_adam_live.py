"""GPU: fbl_sumsq_live / fbl_adam_flat_live (include/fbl_live.h) -- the clip norm and Adam over a live set of the flat buffer.

Dead words carry sentinels (p, m, v: a NaN bit pattern that must survive; g: NaN that must reach nothing).  One range over
the whole buffer must give the bits of fbl_sumsq / fbl_adam_flat; any other pattern, with the clip off, the bits of
fbl_adam_flat run on each live range's slice; with the clip on, the float64 reference within the per-element bound that
tests/test_gpu_rowops.py applies to fbl_adam_flat (imported, not restated).  Two identical calls give identical bits.
"""
import math

import pytest
import torch

from tests import rowop_cases as RC
from tests.gpu_refs import ref_adam
from tests.test_gpu_rowops import AEPS, B1, B2, C_ADAM, LR, SENT, U, exact, judge

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
# n = 8, 24, 4096 + 8, and one size behind which every grid-stride loop wraps (5 x the grid1d cap, as rowop_cases.BIG_N)
SIZES = [8, 24, 4096 + 8, 5 * RC.GRID1D_BLOCK * RC.GRID1D_CAP + 8]
PATTERNS = ["all", "first_dead", "last_dead", "alternating8", "single8_middle"]
WD = 0.01


def ranges_of(pattern, n):
    blocks = n // 8
    if pattern == "all":
        return [(0, n)]
    if pattern == "first_dead":
        return [(8, n)] if blocks > 1 else None
    if pattern == "last_dead":
        return [(0, n - 8)] if blocks > 1 else None
    if pattern == "alternating8":  # 8 live, 8 dead, ..: as many ranges as the table takes, then one live stretch to the end
        if blocks < 3:
            return None
        r = [(16 * i, 16 * i + 8) for i in range(min((blocks + 1) // 2, 1000))]
        if r[-1][1] + 8 < n:
            r.append((r[-1][1] + 8, n))
        return r
    mid = (blocks // 2) * 8
    return [(mid, mid + 8)] if blocks >= 3 else None


CASES = [(n, p) for n in SIZES for p in PATTERNS if ranges_of(p, n) is not None]


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


def live_mask(ranges, n):
    mk = torch.zeros(n, dtype=torch.bool, device=DEV)
    for b, e in ranges:
        mk[b:e] = True
    return mk


def data(n, seed):
    g_ = torch.Generator(device=DEV).manual_seed(seed)
    sign = (torch.randint(0, 2, (n,), generator=g_, device=DEV) * 2 - 1).float()
    mag = lambda: 0.25 + torch.randn(n, generator=g_, device=DEV).abs()
    return sign * mag(), sign * mag(), sign * 0.05 * mag(), (0.05 * mag()) ** 2  # p, g, m, v (as test_adam's late start)


def poisoned(t, dead):
    t = t.clone()
    t.view(torch.int32)[dead] = SENT[F32]
    return t


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("n,pattern", CASES, ids=[f"n{n}-{p}" for n, p in CASES])
def test_live_kernels(L, n, pattern):
    ranges = ranges_of(pattern, n)
    tab = L.live_table(ranges, n, DEV)
    live = live_mask(ranges, n)
    dead = ~live
    p0, g0, m0, v0 = data(n, 11 + n % 97)
    g = poisoned(g0, dead)  # NaN in every dead gradient word
    nws = L.load().fbl_sumsq_ws_floats()
    step = 7

    def run_live(max_norm):
        p, m, v = poisoned(p0, dead), poisoned(m0, dead), poisoned(v0, dead)
        ss = torch.zeros(1, device=DEV)
        ws = torch.full((nws,), float("nan"), device=DEV)
        L.sumsq_live(g, tab, ss, ws)
        L.adam_flat_live(p, g, m, v, tab, LR, B1, B2, AEPS, WD, step, sumsq_t=ss if max_norm > 0 else None, max_norm=max_norm)
        torch.cuda.synchronize()
        return p, m, v, ss

    # ---- clip off: the bits of fbl_adam_flat on each live range's slice (the whole buffer when there is one range over it)
    p, m, v, ss = run_live(0.0)
    for t, t0 in ((p, p0), (m, m0), (v, v0)):
        assert bool((bits(t)[dead] == SENT[F32]).all()), f"{pattern}: a dead word was written"
        assert bool(torch.isfinite(t[live]).all()), f"{pattern}: a dead gradient reached a live result"
    assert bool(torch.isfinite(ss).all())
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    if len(ranges) <= 300:
        for b, e in ranges:
            L.adam_flat(pr[b:e], g[b:e], mr[b:e], vr[b:e], LR, B1, B2, AEPS, WD, step)
    else:  # a thousand slices: one call over the whole buffer instead (element-wise: the live elements see the same operands)
        L.adam_flat(pr, g0, mr, vr, LR, B1, B2, AEPS, WD, step)
    torch.cuda.synchronize()
    for what, t, r in (("p", p, pr), ("m", m, mr), ("v", v, vr)):
        exact(f"{pattern} n={n} {what} vs fbl_adam_flat on the live slices", t[live], r[live])
    # ---- the norm: an exact integer sum would hide the order, so compare with float64 within fbl_sumsq's own bound, and for
    # one whole-buffer range with fbl_sumsq's bits
    sq = (g0.double() ** 2)[live]
    tot = float(sq.sum())
    assert abs(float(ss) - tot) <= 2.0 * int(live.sum()) * U * tot + 2.0 * U * tot
    if pattern == "all":
        s2 = torch.zeros(1, device=DEV)
        L.sumsq(g0, s2, ws=torch.empty(nws, device=DEV))
        exact("one range: fbl_sumsq's bits", ss, s2)
        pw, mw, vw = p0.clone(), m0.clone(), v0.clone()
        L.adam_flat(pw, g0, mw, vw, LR, B1, B2, AEPS, WD, step, sumsq_t=s2, max_norm=0.5 * math.sqrt(tot))
        pc, mc, vc, _ = run_live(0.5 * math.sqrt(tot))
        for what, t, r in (("p", pc, pw), ("m", mc, mw), ("v", vc, vw)):
            exact(f"one range, clip on: fbl_adam_flat's {what}", t, r)
    # ---- clip on (the norm sits above max_norm): float64 reference, test_adam's per-element bound
    max_norm = 0.5 * math.sqrt(tot)
    pc, mc, vc, ssc = run_live(max_norm)
    clip = min(1.0, max_norm / (math.sqrt(tot) + 1e-6))
    assert clip < 1.0
    p64, m64, v64 = p0.double(), m0.double(), v0.double()
    ref_adam(p64, torch.where(live, g0, torch.zeros_like(g0)).double(), m64, v64, lr=LR, b1=B1, b2=B2, eps=AEPS, wd=WD, step=step,
             clip=clip)
    for t in (pc, mc, vc):
        assert bool((bits(t)[dead] == SENT[F32]).all()), f"{pattern}: a dead word was written (clip on)"
    judge(f"adam_live p n={n} {pattern}", pc[live], p64[live], U * (p0.double().abs()[live] + LR), C_ADAM)
    # ---- two identical calls: identical bits
    pd, md, vd, ssd = run_live(max_norm)
    assert torch.equal(bits(ssd), bits(ssc)) and torch.equal(bits(pd), bits(pc)) and torch.equal(bits(md), bits(mc)) \
        and torch.equal(bits(vd), bits(vc)), f"{pattern}: not reproducible bit for bit"


def test_a_malformed_table_is_refused_on_the_host(L):
    for bad in ([(0, 12)], [(8, 16), (0, 8)], [(0, 16), (8, 24)], [(0, 8), (8, 8)], [(0, 40)]):
        with pytest.raises(ValueError):
            L.live_table(bad, 32, "cpu")
    assert L.live_table([(0, 8), (16, 32)], 32, "cpu").tolist() == [2, 24, 0, 0, 16, 8]
