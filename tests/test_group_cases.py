"""CPU: the case table of tests/group_cases.py is what it says it is, and its float64 reference `ref_adam_groups` IS Adam with
parameter groups: three steps in float64 with a clip that bites against torch.optim.Adam over the same segments as separate
parameters in several param_groups -- coupled and decoupled (`decoupled_weight_decay=True`) decay, different betas and eps,
a group with weight_decay = 0.  Tolerance 1e-12 relative: both sides are float64 and differ only in the order of a few
operations (torch forms lr / bc1 and the decay factor in Python floats, and fuses nothing)."""
import math

import pytest
import torch

from tests import group_cases as GC

LR, B1, B2, EPS, WD = 3e-4, 0.9, 0.95, 1e-8, 0.01


def test_the_case_table():
    assert len(GC.CASES) == len({GC.case_id(c) for c in GC.CASES})
    seen_layouts, seen_patterns, most = set(), set(), 0
    for n, lay, pat in GC.CASES:
        segs = GC.case_segments(n, lay, pat)
        live = GC.live_ranges(pat, n)
        last = 0
        for b, e, k in segs:
            assert last <= b < e <= n and b % 8 == 0 and e % 8 == 0 and 0 <= k < GC.n_groups(lay), (n, lay, pat, b, e, k)
            assert any(lb <= b and e <= le for lb, le in live), "a segment leaves the live set"
            last = e
        for (b0, e0, k0), (b1, e1, k1) in zip(segs, segs[1:]):
            assert e0 < b1 or k0 != k1, "neighbours of one group are merged"
        assert sum(e - b for b, e, _ in segs) == sum(e - b for b, e in live), "every live element is in a segment"
        assert len(segs) <= GC.MAX_SEGMENTS
        most = max(most, len(segs))
        seen_layouts.add(lay)
        seen_patterns.add(pat)
    assert seen_layouts == set(GC.LAYOUTS) and seen_patterns == set(GC.PATTERNS)
    assert most == GC.MAX_SEGMENTS  # the limit is reached
    big = GC.case_segments(GC.GRID_WRAP_N, "rr64", "all")
    assert {k for _, _, k in big} == set(range(GC.MAX_GROUPS))
    assert GC.GRID_WRAP_N // 4 > 2 * 2048 * 256  # more than two trips of a 2048-block grid-stride loop, 4 elements per lane
    assert GC.case_segments(8, "two", "all") is None and GC.case_segments(8, "one", "first_dead") is None
    assert GC.case_segments(24, "two", "all") == [(0, 8, 0), (8, 24, 1)]
    assert GC.case_segments(48, "alt8", "alternating8") == [(0, 8, 0), (16, 24, 0), (32, 40, 0)]
    assert GC.case_segments(32, "rr64", "first_dead") == [(8, 16, 1), (16, 24, 2), (24, 32, 3)]
    hy = GC.hyper(4, LR, B1, B2, EPS, WD, "odd")
    assert len({h[:5] for h in hy}) == 4 and [h[5] for h in hy] == [False, True, False, True]
    assert hy[1][4] == 0.0 and all(0.5 * LR < h[0] <= LR for h in hy)


@pytest.mark.parametrize("decoupled", ["none", "odd", "all"])
@pytest.mark.parametrize("n,layout,pattern", [(24, "two", "all"), (4104, "alt8", "first_dead"), (4104, "rr64", "alternating8"),
                                              (4104, "one", "alternating8")])
def test_reference_is_torch_adam_with_param_groups(n, layout, pattern, decoupled):
    segs = GC.case_segments(n, layout, pattern)
    ng = GC.n_groups(layout)
    hy = GC.hyper(ng, LR, B1, B2, EPS, WD, decoupled)
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    grads = [torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(3)]
    live = torch.zeros(n, dtype=torch.bool)
    for b, e, _ in segs:
        live[b:e] = True
    # torch: every segment a parameter of its own, in the param_group of its group
    params = [torch.nn.Parameter(p0[b:e].clone()) for b, e, _ in segs]
    groups = []
    for k, (lr, b1, b2, eps, wd, dec) in enumerate(hy):
        mine = [q for q, (_, _, kk) in zip(params, segs) if kk == k]
        if mine:
            groups.append(dict(params=mine, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, decoupled_weight_decay=dec))
    opt = torch.optim.Adam(groups, lr=1.0, foreach=False)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step, g in enumerate(grads, 1):
        norm = math.sqrt(float((g[live] ** 2).sum()))
        max_norm = 0.5 * norm  # bites at every step
        for q, (b, e, _) in zip(params, segs):
            q.grad = g[b:e].clone()
        total = torch.nn.utils.clip_grad_norm_(params, max_norm)
        assert abs(float(total) - norm) <= 1e-12 * norm
        opt.step()
        clip = min(1.0, max_norm / (norm + 1e-6))
        assert clip < 1.0
        GC.ref_adam_groups(p, g, m, v, segs, hy, step=step, clip=clip)
    assert torch.equal(p[~live], p0[~live]) and not bool(m[~live].any()) and not bool(v[~live].any())
    for q, (b, e, _) in zip(params, segs):
        want = q.detach()
        st = opt.state[q]
        assert float((p[b:e] - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert float((m[b:e] - st["exp_avg"]).abs().max()) <= 1e-12 * float(st["exp_avg"].abs().max())
        assert float((v[b:e] - st["exp_avg_sq"]).abs().max()) <= 1e-12 * float(st["exp_avg_sq"].abs().max())
    assert bool((p[live] != p0[live]).all())
