"""The moving average of fbl_adam_flat_groups_ema (include/fbl_ema.h): its weight schedule, a float64 reference of one update and
the judge, in numpy only -- shared by tests/test_ema_cases.py (which checks these tools), tests/test_gpu_adam_ema.py and
tests/test_gpu_ema_model.py; importable without a GPU.

The kernel forms, in fp32 with contraction off,
    d = p - e          one rounding:  d = (p - e)(1 + a),         |a| <= 2^-24
    e' = fma(w, d, e)  one rounding:  e' = (e + w d)(1 + b),      |b| <= 2^-24
so against ref = e + w (p - e) in exact arithmetic
    e' - ref = w (p - e) a + (ref + w (p - e) a) b,   |e' - ref| <= 2^-24 (w |p - e| + |ref|) + 2^-48 w |p - e|.
The judge's bound is that, with the second-order term (and the float64 evaluation of ref, 2^-53 relative) inside a factor
1 + 2^-20:
    |got - ref| <= 2^-24 (w |p - e| + |ref|) (1 + 2^-20).
Nothing in it was measured.  `w` is the fp32 number the launch receives; e, p are the fp32 inputs; everything else is float64.
"""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20


def weight(d, u, warmup=False):
    """weight of the new parameters in update u = 1, 2, ..: 1 - d, or with warm-up 1 - min(d, (1 + u) / (10 + u))"""
    assert u >= 1
    return 1.0 - (min(d, (1.0 + u) / (10.0 + u)) if warmup else d)


def w32(w):
    """the weight as the launch sees it: rounded to fp32, as a Python float"""
    return float(np.float32(w))


def _f64(x):
    if hasattr(x, "detach"):  # a torch tensor, wherever it lives
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(np.float64)


def ref_update(e, p, w):
    """e + w (p - e) in float64 on the fp32 inputs (w: the fp32 weight)"""
    e, p = _f64(e), _f64(p)
    return e + w32(w) * (p - e)


def bound(e, p, w):
    """the per-element bound of one update (module docstring)"""
    e, p = _f64(e), _f64(p)
    w = w32(w)
    return U * (w * np.abs(p - e) + np.abs(e + w * (p - e))) * SLACK


def outside(got, e, p, w):
    """(elements outside the bound, worst error in units of the bound)"""
    err = np.abs(_f64(got) - ref_update(e, p, w))
    b = bound(e, p, w)
    err = np.where(np.isnan(err), np.inf, err)
    bad = err > b
    ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0


def judge(what, got, e, p, w):
    """no element of `got` may be outside the bound; the worst ratio is printed before the assertion"""
    n_bad, worst = outside(got, e, p, w)
    print(f"{what}: worst error {worst:.3f} of the bound, {n_bad} outside")
    assert n_bad == 0, f"{what}: {n_bad} elements outside the bound, worst {worst:.3f} x"


def emulate(e, p, w):
    """the kernel's two instructions in numpy: an fp32 subtraction, then the fma as a float64 product and sum (exact up to the
    one rounding of the float64 sum: fp32 x fp32 fits float64) rounded to fp32"""
    e = np.asarray(e, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    d = (p - e).astype(np.float32)
    return (np.float64(np.float32(w)) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)


def recurrence(e0, ps, ws):
    """float64: the average after the updates (p_1, w_1), (p_2, w_2), ..  (ws: the fp32 weights)"""
    e = _f64(e0)
    for p, w in zip(ps, ws):
        e = e + w32(w) * (_f64(p) - e)
    return e


def closed_form(e0, ps, ws):
    """the same average written out: e_n = prod(1 - w_k) e_0 + sum_k w_k prod_{j > k}(1 - w_j) p_k"""
    ws = [w32(w) for w in ws]
    out = _f64(e0) * np.prod([1.0 - w for w in ws])
    for k, p in enumerate(ps):
        out = out + ws[k] * np.prod([1.0 - w for w in ws[k + 1:]]) * _f64(p)
    return out


def accumulated_bound(es, ps, ws):
    """Bound on |kernel's average - recurrence| after the updates (p_k, w_k), from the per-update one.  es[k] is the KERNEL's
    average in front of update k (es[0] = e_0, shared with the recurrence).  One update maps the reference r and the kernel's e by
    the same affine map up to the kernel's rounding: |e_k - r_k| <= (1 - w_k) |e_{k-1} - r_{k-1}| + bound(e_{k-1}, p_k, w_k)."""
    B = np.zeros_like(_f64(es[0]))
    for e, p, w in zip(es, ps, ws):
        B = (1.0 - w32(w)) * B + bound(e, p, w)
    return B
