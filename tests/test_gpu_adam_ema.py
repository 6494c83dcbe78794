"""GPU: fbl_adam_flat_groups_ema and fbl_swap_f32 (include/fbl_ema.h) -- Adam over parameter groups with the moving average of
the updated parameter in the same launch -- on the sizes, group layouts and live patterns of tests/group_cases.py (imported) and
two more: n = 8 with one segment (the smallest legal buffer) and a two-group layout with a dead head and a dead stretch in the
middle whose last segment ends at n.

Dead words carry sentinels in all five buffers (p, m, v, ema: a NaN bit pattern that must survive; g: NaN that must reach nothing),
as in tests/test_gpu_adam_groups.py.  Every case runs three consecutive steps with ema_w from the warm-up schedule of decay 0.999
(1 - 2/11, 1 - 3/12, 1 - 4/13) and one step with ema_w = 1 - 0.999; groups: all coupled, and -- where there are several -- every
other one decoupled; the clip bites.  Conditions:
 1. p, m, v carry the bits of fbl_adam_flat_groups run on copies (whole buffers, sentinels included); over the whole buffer with
    one coupled group the bits of fbl_adam_flat;
 2. every live element of ema passes the judge of tests/ema_cases.py -- |got - ref| <= 2^-24 (w |p - e| + |ref|) (1 + 2^-20)
    against ref = e + w (p - e) in float64, p the kernel's own output -- no element outside;
 3. every dead word of ema keeps its sentinel, and no dead p or g reaches a live result;
 4. where ema == p_new going in, ema keeps its bits;
 5. a segment with a group id out of range touches nothing;
 6. two identical calls give identical bits;
 7. fbl_swap_f32 exchanges two buffers exactly for n in {8, 4104, 30_000_008}, NaN payloads and -0.0 included; swapping twice is
    the identity.

On the parent commit every test fails at its first call into the binding: module 'frozenbilm_amd.lib' has no attribute
'adam_flat_groups_ema' / 'swap_' (seen there; it has no include/fbl_ema.h to bind)."""
import math

import pytest
import torch

from tests import ema_cases as EC
from tests import group_cases as GC
from tests.test_gpu_adam_groups import bits, data, masks, poisoned
from tests.test_gpu_rowops import AEPS, B1, B2, LR, SENT, exact

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
WD = 0.01
STEP = 7
DECAY = 0.999

# (id, n, segments, groups): the cases of tests/group_cases.py, then the two of this file
CASES = [(GC.case_id(c), c[0], GC.case_segments(*c), GC.n_groups(c[1])) for c in GC.CASES]
CASES += [("n8-one-segment", 8, [(0, 8, 0)], 1),
          ("n4104-last-segment-ends-at-n", 4096 + 8, [(8, 1024, 1), (1024, 2048, 0), (2056, 4096 + 8, 1)], 2)]


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


class Setup:
    def __init__(self, L, n, segs, ng):
        self.L, self.n, self.segs, self.ng = L, n, segs, ng
        self.tab = L.group_table(segs, n, DEV, ng)
        self.live, self.grp = masks(segs, n)
        self.dead = ~self.live
        assert int(self.live.sum()) == sum(e - b for b, e, _ in segs)
        self.p0, self.g0, self.m0, self.v0 = data(n, 11 + n % 97)
        # the average going in: near the parameter, as after some updates (a few Adam steps of size LR away), not equal to it
        gen = torch.Generator(device=DEV).manual_seed(5 + n % 89)
        self.e0 = self.p0 + 4 * LR * torch.randn(n, generator=gen, device=DEV)
        self.g = poisoned(self.g0, self.dead)  # NaN in every dead gradient word
        ranges = []
        for b, e, _ in segs:
            if ranges and ranges[-1][1] == b:
                ranges[-1] = (ranges[-1][0], e)
            else:
                ranges.append((b, e))
        self.ss = torch.zeros(1, device=DEV)  # the ONE norm: over the live elements of all groups
        L.sumsq_live(self.g, L.live_table(ranges, n, DEV), self.ss, torch.empty(L.load().fbl_sumsq_ws_floats(), device=DEV))
        self.tot = float((self.g0.double() ** 2)[self.live].sum())
        self.max_norm = 0.5 * math.sqrt(self.tot)  # bites
        assert abs(float(self.ss) - self.tot) <= 1e-4 * self.tot

    def start(self):
        return [poisoned(t, self.dead) for t in (self.p0, self.m0, self.v0, self.e0)]

    def step(self, state, hyper, step, w, what, tab=None):
        """one launch on `state` = [p, m, v, ema] in place, next to fbl_adam_flat_groups on copies: conditions 1, 2, 3"""
        L = self.L
        p, m, v, ema = state
        pc, mc, vc, e_in = p.clone(), m.clone(), v.clone(), ema.clone()
        kw = dict(sumsq_t=self.ss, max_norm=self.max_norm)
        L.adam_flat_groups(pc, self.g, mc, vc, self.tab if tab is None else tab, hyper, step, **kw)
        L.adam_flat_groups_ema(p, self.g, m, v, ema, self.tab if tab is None else tab, hyper, step, w, **kw)
        torch.cuda.synchronize()
        for nm, t, r in (("p", p, pc), ("m", m, mc), ("v", v, vc)):
            exact(f"{what}: {nm} vs fbl_adam_flat_groups", t, r)
        for nm, t in (("p", p), ("m", m), ("v", v), ("ema", ema)):
            assert bool((bits(t)[self.dead] == SENT[F32]).all()), f"{what}: a dead word of {nm} was written"
            assert bool(torch.isfinite(t[self.live]).all()), f"{what}: a dead word reached a live result of {nm}"
        EC.judge(f"{what}: ema", ema[self.live], e_in[self.live], p[self.live], w)
        return e_in


@pytest.mark.parametrize("cid,n,segs,ng", CASES, ids=[c[0] for c in CASES])
def test_ema_kernel(L, cid, n, segs, ng):
    s = Setup(L, n, segs, ng)
    live = s.live
    # one group: coupled; several: every other one decoupled next to coupled neighbours (small sizes: all coupled as well)
    for mode in (("none",) if ng == 1 else ("odd",) if n > 1 << 20 else ("none", "odd")):
        hy = GC.hyper(ng, LR, B1, B2, AEPS, WD, mode)
        # ---- three consecutive steps on the warm-up schedule
        state = s.start()
        for u in (1, 2, 3):
            w = EC.weight(DECAY, u, True)
            e_in = s.step(state, hy, STEP + u - 1, w, f"{cid} {mode} update {u}")
            assert not torch.equal(bits(state[3])[live], bits(e_in)[live]), "the average did not move"
        # ---- one step with ema_w = 1 - 0.999
        w = EC.weight(DECAY, 1, False)
        assert w == 1.0 - 0.999
        state = s.start()
        s.step(state, hy, STEP, w, f"{cid} {mode} w=1-0.999")
        # ---- 6. two identical calls: identical bits
        again = s.start()
        L.adam_flat_groups_ema(*again[:1], s.g, *again[1:], s.tab, hy, STEP, w, sumsq_t=s.ss, max_norm=s.max_norm)
        torch.cuda.synchronize()
        for a, b in zip(again, state):
            assert torch.equal(bits(a), bits(b)), f"{cid}: not reproducible bit for bit"
        # ---- 4. where ema == p_new going in it keeps its bits (everywhere, then on every other live 8-block)
        p_new = state[0]
        for every_other in (False, True):
            eq = live.clone()
            if every_other:
                eq &= (torch.arange(n, device=DEV) // 8) % 2 == 0
            e_start = torch.where(eq, p_new, poisoned(s.e0, s.dead))
            st = s.start()
            st[3] = e_start.clone()
            L.adam_flat_groups_ema(st[0], s.g, st[1], st[2], st[3], s.tab, hy, STEP, w, sumsq_t=s.ss, max_norm=s.max_norm)
            torch.cuda.synchronize()
            exact(f"{cid}: p of the run that starts with ema == p_new", st[0], p_new)
            assert torch.equal(bits(st[3])[eq], bits(p_new)[eq]), f"{cid}: ema == p_new going in changed its bits"
            rest = live & ~eq
            if bool(rest.any()):
                EC.judge(f"{cid}: the other elements", st[3][rest], e_start[rest], p_new[rest], w)
    # ---- 1b. one coupled group over the whole buffer: the bits of fbl_adam_flat
    if ng == 1 and segs == [(0, n, 0)]:
        lr, b1, b2, eps, wd, _ = hy[0]
        p, m, v, ema = s.start()
        pw, mw, vw = s.p0.clone(), s.m0.clone(), s.v0.clone()
        for clip in (False, True):
            kw = dict(sumsq_t=s.ss, max_norm=s.max_norm) if clip else {}
            L.adam_flat_groups_ema(p, s.g, m, v, ema, s.tab, hy, STEP, 0.5, **kw)
            L.adam_flat(pw, s.g0, mw, vw, lr, b1, b2, eps, wd, STEP, **kw)
            torch.cuda.synchronize()
            for nm, t, r in (("p", p, pw), ("m", m, mw), ("v", v, vw)):
                exact(f"{cid} clip={clip}: {nm} vs fbl_adam_flat", t, r)


@pytest.mark.parametrize("n", [24, 4096 + 8])
def test_a_group_id_out_of_range_touches_nothing(L, n):
    """condition 5: lib.group_table refuses such a table, so it is written by hand -- segment 1 names group 2 of 2, group -1 and
    2^40; its words keep their sentinels in all five buffers, the other segment is updated as if it were dead"""
    segs = GC.case_segments(n, "two", "all")
    s = Setup(L, n, segs, 2)
    assert len(segs) == 2
    hy = GC.hyper(2, LR, B1, B2, AEPS, WD, "odd")
    w = EC.weight(DECAY, 2, True)
    want = s.start()
    L.adam_flat_groups_ema(want[0], s.g, want[1], want[2], want[3], s.tab, hy, STEP, w, sumsq_t=s.ss, max_norm=s.max_norm)
    (b0, e0, _), (b1, e1, _) = segs
    for bad in (2, -1, 1 << 40):
        tab = torch.tensor([2, n, b0, 0, 0, b1, e0 - b0, bad], dtype=torch.int64, device=DEV)
        st = s.start()
        g = s.g.clone()
        for t in (*st, g):
            bits(t)[b1:e1] = SENT[F32]
        L.adam_flat_groups_ema(st[0], g, st[1], st[2], st[3], tab, hy, STEP, w, sumsq_t=s.ss, max_norm=s.max_norm)
        torch.cuda.synchronize()
        for t, wt in zip(st, want):
            assert bool((bits(t)[b1:e1] == SENT[F32]).all()), f"group id {bad}: the segment was touched"
            exact(f"group id {bad}: the other segment", t[b0:e0], wt[b0:e0])


def test_the_binding_refuses_bad_arguments(L):
    p, g, m, v, ema = (torch.zeros(16, device=DEV) for _ in range(5))
    tab = L.group_table([(0, 16, 0)], 16, DEV, 1)
    hy = [(LR, B1, B2, AEPS, 0.0, False)]
    for w in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            L.adam_flat_groups_ema(p, g, m, v, ema, tab, hy, 1, w)
    with pytest.raises(ValueError):
        L.adam_flat_groups_ema(p, g, m, v, torch.zeros(24, device=DEV), tab, hy, 1, 0.1)
    with pytest.raises(TypeError):
        L.adam_flat_groups_ema(p, g, m, v, ema.double(), tab, hy, 1, 0.1)
    with pytest.raises(ValueError):
        L.adam_flat_groups_ema(p, g, m, v, torch.zeros(24, device=DEV)[2:18], tab, hy, 1, 0.1)  # 8 bytes off a 16-byte boundary
    big = torch.zeros(32, device=DEV)
    for a, b in ((p, p), (big[:16], big[8:24]), (p, big), (p, big[2:18])):
        with pytest.raises(ValueError):
            L.swap_(a, b)
    with pytest.raises(TypeError):
        L.swap_(p, g.half())
    torch.cuda.synchronize()
    assert not bool(p.any()) and not bool(ema.any())


@pytest.mark.parametrize("n", [8, 4096 + 8, 30_000_008])
def test_swap(L, n):
    """condition 7: random bit patterns (NaN payloads, infinities and denormals among them), -0.0 and the sentinel NaN at the
    ends; guard words behind both buffers keep their bits"""
    gen = torch.Generator(device=DEV).manual_seed(n % 1009)
    G = 8
    bufs = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n + G,), generator=gen, device=DEV, dtype=torch.int64).to(torch.int32)
            for _ in range(2)]
    for t in bufs:
        t[0], t[n - 1], t[1], t[n - 2] = -2 ** 31, SENT[F32], 0x7F800001, -1  # -0.0, NaNs with payloads (signalling, all ones)
    a, b = (t.view(F32) for t in bufs)
    assert bool(torch.isnan(a[:n]).any()) and bool((bufs[0][:n] != bufs[1][:n]).any())
    a0, b0 = bufs[0].clone(), bufs[1].clone()
    L.swap_(a[:n], b[:n])
    torch.cuda.synchronize()
    assert torch.equal(bufs[0][:n], b0[:n]) and torch.equal(bufs[1][:n], a0[:n]), "not exchanged bit for bit"
    assert torch.equal(bufs[0][n:], a0[n:]) and torch.equal(bufs[1][n:], b0[n:]), "a word behind the buffers was written"
    L.swap_(a[:n], b[:n])
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], a0) and torch.equal(bufs[1], b0), "swapping twice is not the identity"
