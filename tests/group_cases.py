"""Case table and float64 reference of fbl_adam_flat_groups (include/fbl_groups.h); importable without a GPU.

A case is (n, layout, pattern): `layout` says which parameter group every 8-element block of the flat buffer belongs to,
`pattern` which blocks are live; `case_segments` cuts the two into the (begin, end, group) segments the kernel walks -- at most
1024: where a layout would give more, the groups alternate up to the limit and one group takes the rest.  tests/test_group_cases.py
checks the table and holds `ref_adam_groups` against torch.optim.Adam with several param_groups.
"""
from tests.gpu_refs import ref_adam

MAX_SEGMENTS = 1024
MAX_GROUPS = 64
GRID_WRAP_N = 5 * 256 * 4096 + 8  # wraps the grid-stride loop of a 2048-block, 4-element-per-lane kernel more than twice
SIZES = [8, 24, 4096 + 8, GRID_WRAP_N]
LAYOUTS = ["one", "two", "alt8", "rr64"]
PATTERNS = ["all", "first_dead", "alternating8"]


def n_groups(layout):
    return {"one": 1, "two": 2, "alt8": 2, "rr64": MAX_GROUPS}[layout]


def live_ranges(pattern, n):
    """the live [begin, end) ranges, or None where the pattern needs more blocks than n has (the patterns of
    tests/test_gpu_adam_live.py)"""
    blocks = n // 8
    if pattern == "all":
        return [(0, n)]
    if pattern == "first_dead":
        return [(8, n)] if blocks > 1 else None
    assert pattern == "alternating8"  # 8 live, 8 dead, ..: a thousand ranges, then one live stretch to the end
    if blocks < 3:
        return None
    r = [(16 * i, 16 * i + 8) for i in range(min((blocks + 1) // 2, 1000))]
    if r[-1][1] + 8 < n:
        r.append((r[-1][1] + 8, n))
    return r


def _run(layout, i, blocks):
    """(group of block i, the first block behind i's run of that group)"""
    if layout == "one":
        return 0, blocks
    if layout == "two":
        mid = blocks // 2
        return (0, mid) if i < mid else (1, blocks)
    if layout == "alt8":
        return i % 2, i + 1
    assert layout == "rr64"
    return i % MAX_GROUPS, i + 1


def case_segments(n, layout, pattern):
    """sorted, disjoint, 8-aligned (begin, end, group) segments: maximal runs that are live and of one group; None where the
    case does not exist (too few blocks for the pattern, or for the layout to show a second group)"""
    ranges = live_ranges(pattern, n)
    blocks = n // 8
    if ranges is None or (layout != "one" and blocks < 2):
        return None
    segs, tail = [], None
    for r, (b, e) in enumerate(ranges):
        i, end = b // 8, e // 8
        while i < end:
            later = len(ranges) - 1 - r  # every later range needs a segment of its own
            if tail is None and len(segs) + later >= MAX_SEGMENTS - 1:
                tail = _run(layout, i, blocks)[0]  # the limit: this group takes whatever is left
            k, stop = (tail, end) if tail is not None else _run(layout, i, blocks)
            stop = min(stop, end)
            if segs and segs[-1][1] == 8 * i and segs[-1][2] == k:
                segs[-1] = (segs[-1][0], 8 * stop, k)
            else:
                segs.append((8 * i, 8 * stop, k))
            i = stop
    assert 1 <= len(segs) <= MAX_SEGMENTS
    return segs


CASES = [(n, lay, pat) for n in SIZES for lay in LAYOUTS for pat in PATTERNS if case_segments(n, lay, pat) is not None]


def case_id(c):
    return f"n{c[0]}-{c[1]}-{c[2]}"


def hyper(ng, lr, b1, b2, eps, wd, decoupled="none"):
    """`ng` records (lr, beta1, beta2, eps, weight_decay, decoupled), all different: rates in (lr / 2, lr], betas at and below
    (b1, b2), epsilons at and above eps, weight decays 0 (group 1, where there is one), wd, 2 wd, ...; decoupled: "none", "all"
    or "odd" (the groups 1, 3, ..)"""
    out = []
    for k in range(ng):
        f = (k + 1) / ng
        dec = {"none": False, "all": True, "odd": k % 2 == 1}[decoupled]
        out.append((lr * (0.5 + 0.5 * f), b1 - 0.2 * (1.0 - f), b2 - 0.1 * (1.0 - f), eps * (1.0 + 3.0 * (1.0 - f)),
                    0.0 if (k == 1 and ng > 1) else wd * (1 + k % 3), dec))
    return out


def ref_adam_groups(p, g, m, v, segments, groups, *, step, clip):
    """One fbl_adam_flat_groups step in float64, in place on the segments of p / m / v (float64 tensors; g is read).  groups[k] =
    (lr, beta1, beta2, eps, weight_decay, decoupled).  A coupled group: ref_adam (L2 decay folded into the gradient).  A
    decoupled one: p <- p * (1 - lr * wd) first, then ref_adam with no decay (torch.optim.AdamW).  `clip` is the one factor of
    the global norm (times grad_scale), the same for every group.  Elements outside the segments are left alone."""
    for b, e, k in segments:
        lr, b1, b2, eps, wd, dec = groups[k]
        ps, ms, vs = p[b:e], m[b:e], v[b:e]  # (views: updated in place)
        if dec:
            ps.mul_(1.0 - lr * wd)
        ref_adam(ps, g[b:e], ms, vs, lr=lr, b1=b1, b2=b2, eps=eps, wd=0.0 if dec else wd, step=step, clip=clip)
