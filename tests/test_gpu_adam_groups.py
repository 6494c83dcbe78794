"""GPU: fbl_adam_flat_groups (include/fbl_groups.h) -- Adam over parameter groups of the flat buffer, on the cases of
tests/group_cases.py (sizes x group layouts x live patterns).

Dead words carry sentinels (p, m, v: a NaN bit pattern that must survive; g: NaN that must reach nothing), as in
tests/test_gpu_adam_live.py.  Conditions:
 1. one coupled group: the bits of fbl_adam_flat_live on the same ranges, and over the whole buffer the bits of fbl_adam_flat;
 2. several coupled groups with different lr / betas / eps / wd: the bits of fbl_adam_flat run on each segment's slice with
    its group's values -- with the clip off, and with the clip on and the one shared norm handed to every slice call (beyond 64
    segments: one fbl_adam_flat call per GROUP over the whole buffer, the group's elements taken from it -- the update is
    element-wise, the live elements see the same operands);
 3. decoupled groups: the float64 reference group_cases.ref_adam_groups within the per-element bound U (|p| + LR) C_ADAM that
    tests/test_gpu_rowops.py applies to fbl_adam_flat (imported, not restated; every group's rate is at most LR);
 4. no dead word is written, no dead gradient reaches a live result;
 5. a segment whose group id is out of range touches nothing;
 6. two identical calls give identical bits.

On the parent commit every test fails at its first line, in `Setup`: module 'frozenbilm_amd.lib' has no attribute
'group_table' (seen there for lib.group_table on the CPU, tests/test_groups_abi.py; there is no fbl_adam_flat_groups to bind)."""
import math

import pytest
import torch

from tests import group_cases as GC
from tests.test_gpu_rowops import AEPS, B1, B2, C_ADAM, LR, SENT, U, exact, judge

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
WD = 0.01
STEP = 7


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


def data(n, seed):
    g_ = torch.Generator(device=DEV).manual_seed(seed)
    sign = (torch.randint(0, 2, (n,), generator=g_, device=DEV) * 2 - 1).float()
    mag = lambda: 0.25 + torch.randn(n, generator=g_, device=DEV).abs()  # noqa: E731
    return sign * mag(), sign * mag(), sign * 0.05 * mag(), (0.05 * mag()) ** 2  # p, g, m, v (as test_adam's late start)


def poisoned(t, dead):
    t = t.clone()
    t.view(torch.int32)[dead] = SENT[F32]
    return t


def bits(t):
    return t.view(torch.int32)


def masks(segs, n):
    """(live mask, group of every element; -1 where dead)"""
    grp = torch.full((n,), -1, dtype=torch.int32)
    b = torch.tensor([s[0] for s in segs])
    e = torch.tensor([s[1] for s in segs])
    k = torch.tensor([s[2] for s in segs], dtype=torch.int32)
    mark = torch.zeros(n + 1, dtype=torch.int32)  # +k+1 at a begin, -(k+1) at an end: the running sum is group + 1 inside
    mark.index_add_(0, b, k + 1)
    mark.index_add_(0, e, -(k + 1))
    grp = (mark.cumsum(0)[:n] - 1).to(torch.int32).to(DEV)
    return grp >= 0, grp


class Setup:
    def __init__(self, L, n, layout, pattern):
        self.L, self.n = L, n
        self.segs = GC.case_segments(n, layout, pattern)
        self.ng = GC.n_groups(layout)
        self.tab = L.group_table(self.segs, n, DEV, self.ng)
        self.live, self.grp = masks(self.segs, n)
        self.dead = ~self.live
        assert int(self.live.sum()) == sum(e - b for b, e, _ in self.segs)
        self.p0, self.g0, self.m0, self.v0 = data(n, 11 + n % 97)
        self.g = poisoned(self.g0, self.dead)  # NaN in every dead gradient word
        self.ranges = []
        for b, e, _ in self.segs:
            if self.ranges and self.ranges[-1][1] == b:
                self.ranges[-1] = (self.ranges[-1][0], e)
            else:
                self.ranges.append((b, e))
        self.live_tab = L.live_table(self.ranges, n, DEV)
        self.ss = torch.zeros(1, device=DEV)  # the ONE norm: over the live elements of all groups
        L.sumsq_live(self.g, self.live_tab, self.ss, torch.empty(L.load().fbl_sumsq_ws_floats(), device=DEV))
        self.tot = float((self.g0.double() ** 2)[self.live].sum())
        self.max_norm = 0.5 * math.sqrt(self.tot)  # bites
        assert abs(float(self.ss) - self.tot) <= 1e-4 * self.tot and bool(torch.isfinite(self.ss).all())

    def run(self, hyper, clip, tab=None):
        p, m, v = poisoned(self.p0, self.dead), poisoned(self.m0, self.dead), poisoned(self.v0, self.dead)
        self.L.adam_flat_groups(p, self.g, m, v, self.tab if tab is None else tab, hyper, STEP, sumsq_t=self.ss if clip else None,
                                max_norm=self.max_norm if clip else 0.0)
        torch.cuda.synchronize()
        for t in (p, m, v):  # condition 4
            assert bool((bits(t)[self.dead] == SENT[F32]).all()), "a dead word was written"
            assert bool(torch.isfinite(t[self.live]).all()), "a dead gradient reached a live result"
        return p, m, v

    def per_slice(self, hyper, clip):
        """fbl_adam_flat with each group's values: on every segment's slice, or -- beyond 64 segments -- once per group over the
        whole buffer, the group's elements taken from the result"""
        L = self.L
        kw = dict(sumsq_t=self.ss, max_norm=self.max_norm) if clip else {}
        pr, mr, vr = self.p0.clone(), self.m0.clone(), self.v0.clone()
        if len(self.segs) <= 64:
            for b, e, k in self.segs:
                lr, b1, b2, eps, wd, _ = hyper[k]
                L.adam_flat(pr[b:e], self.g[b:e], mr[b:e], vr[b:e], lr, b1, b2, eps, wd, STEP, **kw)
        else:
            for k in sorted({s[2] for s in self.segs}):
                lr, b1, b2, eps, wd, _ = hyper[k]
                pk, mk, vk = self.p0.clone(), self.m0.clone(), self.v0.clone()
                L.adam_flat(pk, self.g0, mk, vk, lr, b1, b2, eps, wd, STEP, **kw)
                sel = self.grp == k
                pr[sel], mr[sel], vr[sel] = pk[sel], mk[sel], vk[sel]
        torch.cuda.synchronize()
        return pr, mr, vr


@pytest.mark.parametrize("n,layout,pattern", GC.CASES, ids=[GC.case_id(c) for c in GC.CASES])
def test_group_kernel(L, n, layout, pattern):
    s = Setup(L, n, layout, pattern)
    live = s.live
    what = f"n={n} {layout} {pattern}"
    coupled = GC.hyper(s.ng, LR, B1, B2, AEPS, WD, "none")
    if layout == "one":
        # ---- 1. one coupled group: fbl_adam_flat_live on the same ranges; over the whole buffer fbl_adam_flat
        lr, b1, b2, eps, wd, _ = coupled[0]
        for clip in (False, True):
            p, m, v = s.run(coupled, clip)
            pl, ml, vl = poisoned(s.p0, s.dead), poisoned(s.m0, s.dead), poisoned(s.v0, s.dead)
            L.adam_flat_live(pl, s.g, ml, vl, s.live_tab, lr, b1, b2, eps, wd, STEP, sumsq_t=s.ss if clip else None,
                             max_norm=s.max_norm if clip else 0.0)
            for nm, t, r in (("p", p, pl), ("m", m, ml), ("v", v, vl)):
                exact(f"{what} clip={clip}: {nm} vs fbl_adam_flat_live", t, r)
            if pattern == "all":
                pw, mw, vw = s.p0.clone(), s.m0.clone(), s.v0.clone()
                L.adam_flat(pw, s.g0, mw, vw, lr, b1, b2, eps, wd, STEP, sumsq_t=s.ss if clip else None,
                            max_norm=s.max_norm if clip else 0.0)
                for nm, t, r in (("p", p, pw), ("m", m, mw), ("v", v, vw)):
                    exact(f"{what} clip={clip}: {nm} vs fbl_adam_flat", t, r)
    # ---- 2. coupled groups, each with its own values: fbl_adam_flat per slice, clip off and on (one group: the same check)
    for clip in (False, True):
        p, m, v = s.run(coupled, clip)
        pr, mr, vr = s.per_slice(coupled, clip)
        for nm, t, r in (("p", p, pr), ("m", m, mr), ("v", v, vr)):
            exact(f"{what} clip={clip}: {nm} vs fbl_adam_flat with each group's values", t[live], r[live])
    # ---- 3. decoupled groups (all of them; and every other one next to coupled neighbours): float64 reference
    clipf = min(1.0, s.max_norm / (math.sqrt(s.tot) + 1e-6))
    assert clipf < 1.0
    g64 = torch.where(live, s.g0, torch.zeros_like(s.g0)).double()
    for mode in (("all",) if s.ng == 1 else ("all", "odd")):
        hy = GC.hyper(s.ng, LR, B1, B2, AEPS, WD, mode)
        assert all(h[0] <= LR for h in hy)
        p, m, v = s.run(hy, True)
        p64, m64, v64 = s.p0.double(), s.m0.double(), s.v0.double()
        GC.ref_adam_groups(p64, g64, m64, v64, s.segs, hy, step=STEP, clip=clipf)
        judge(f"adam_groups p {what} decoupled={mode}", p[live], p64[live], U * (s.p0.double().abs()[live] + LR), C_ADAM)
        judge(f"adam_groups m {what} decoupled={mode}", m[live], m64[live], U * (s.m0.double().abs()[live] + g64.abs()[live]), C_ADAM)
        if mode == "odd":  # the coupled groups among them keep fbl_adam_flat's bits
            pr, mr, vr = s.per_slice(hy, True)
            sel = live & (s.grp % 2 == 0)
            exact(f"{what}: coupled groups next to decoupled ones", p[sel], pr[sel])
        # decoupled decay is not the coupled one: where a decoupled group with wd > 0 has a live segment the two differ somewhere
        if any(hy[k][4] > 0 and hy[k][5] for _, _, k in s.segs):
            pc, _, _ = s.run([h[:5] + (False,) for h in hy], True)
            assert not torch.equal(bits(pc)[live], bits(p)[live])
        # ---- 6. two identical calls: identical bits
        p2, m2, v2 = s.run(hy, True)
        assert torch.equal(bits(p2), bits(p)) and torch.equal(bits(m2), bits(m)) and torch.equal(bits(v2), bits(v)), \
            f"{what}: not reproducible bit for bit"


@pytest.mark.parametrize("n", [24, 4096 + 8])
def test_a_group_id_out_of_range_touches_nothing(L, n):
    """condition 5: lib.group_table refuses such a table, so it is written by hand -- segment 1 names group 2 of 2, and (second
    table) group -1; its words keep their sentinels, the other segments are updated as if it were dead"""
    s = Setup(L, n, "two", "all")
    assert len(s.segs) == 2
    hy = GC.hyper(2, LR, B1, B2, AEPS, WD, "odd")
    want_p, want_m, want_v = s.run(hy, True)
    (b0, e0, _), (b1, e1, _) = s.segs
    for bad in (2, -1, 1 << 40):
        tab = torch.tensor([2, n, b0, 0, 0, b1, e0 - b0, bad], dtype=torch.int64, device=DEV)
        p, m, v = poisoned(s.p0, s.dead), s.m0.clone(), s.v0.clone()
        for t in (p, m, v):
            bits(t)[b1:e1] = SENT[F32]
        g = s.g.clone()
        bits(g)[b1:e1] = SENT[F32]
        L.adam_flat_groups(p, g, m, v, tab, hy, STEP, sumsq_t=s.ss, max_norm=s.max_norm)
        torch.cuda.synchronize()
        for t, w in ((p, want_p), (m, want_m), (v, want_v)):
            assert bool((bits(t)[b1:e1] == SENT[F32]).all()), f"group id {bad}: the segment was touched"
            exact(f"group id {bad}: the other segment", t[b0:e0], w[b0:e0])
