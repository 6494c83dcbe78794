"""CPU: the tools of tests/ema_cases.py -- the float64 reference of the moving average, the judge and the weight schedule --
checked against themselves, and optim.ema_weight against the schedule.

 - the reference recurrence over 50 updates equals its closed form;
 - a numpy fp32 emulation of the kernel's two instructions (rounded difference, one fma) passes the judge, whose bound is derived
   in tests/ema_cases.py from those two roundings: |got - ref| <= 2^-24 (w |p - e| + |ref|) (1 + 2^-20), no element outside;
 - the same values moved by 2 ulp fail it;
 - optim.ema_weight gives 1 - d without warm-up and 1 - 2/11, 1 - 3/12, .. with it, capped at 1 - d.

The weights the judge is tried at are the ones the optimizer hands to the launch (optim.ema_weight), so the module needs it.

Seen on the parent commit: the module does not import -- ImportError: cannot import name 'ema_weight' from
'frozenbilm_amd.optim' -- so every test here fails."""
import numpy as np
import pytest

from frozenbilm_amd.optim import ema_weight
from tests import ema_cases as EC


def _data(n, seed):
    r = np.random.default_rng(seed)
    sign = r.integers(0, 2, n) * 2.0 - 1.0
    e = (sign * (0.25 + np.abs(r.standard_normal(n)))).astype(np.float32)
    p = (e + 3e-3 * r.standard_normal(n)).astype(np.float32)  # a parameter a few Adam steps away from its average
    return e, p


def test_recurrence_equals_closed_form():
    r = np.random.default_rng(3)
    e0 = r.standard_normal(257).astype(np.float32)
    ps = [r.standard_normal(257).astype(np.float32) for _ in range(50)]
    for warmup in (False, True):
        ws = [ema_weight(0.9, u, warmup) for u in range(1, 51)]
        a, b = EC.recurrence(e0, ps, ws), EC.closed_form(e0, ps, ws)
        assert np.abs(a - b).max() <= 1e-13 * (1.0 + np.abs(b).max())
    # constant parameters: e_n = p + (1 - w)^n (e_0 - p)
    w = EC.weight(0.99, 1)
    a = EC.recurrence(e0, [ps[0]] * 50, [w] * 50)
    b = ps[0].astype(np.float64) + (1.0 - EC.w32(w)) ** 50 * (e0.astype(np.float64) - ps[0])
    assert np.abs(a - b).max() <= 1e-13 * (1.0 + np.abs(b).max())


@pytest.mark.parametrize("w", [ema_weight(0.999, 1), ema_weight(0.9, 1), ema_weight(0.999, 1, True), 1.0])
def test_emulation_passes_and_two_ulp_fail(w):
    e, p = _data(1 << 16, 5)
    got = EC.emulate(e, p, w)
    n_bad, worst = EC.outside(got, e, p, w)
    assert n_bad == 0 and worst <= 1.0, (n_bad, worst)
    EC.judge(f"emulation w={w}", got, e, p, w)
    if w == 1.0:
        assert np.array_equal(got, p)  # (e + (p - e) = p wherever the difference is exact: these p and e are that close)
    for sign in (1, -1):
        moved = (got.view(np.int32) + 2 * sign).view(np.float32)
        n_bad, worst = EC.outside(moved, e, p, w)
        assert n_bad >= got.size // 2 and worst > 1.0, (w, sign, n_bad, worst)  # (all but mantissas just below a power of two)
        with pytest.raises(AssertionError):
            EC.judge(f"2 ulp off w={w}", moved, e, p, w)
    # where the average equals the parameter it keeps its bits; a NaN is outside whatever the bound
    assert np.array_equal(EC.emulate(p, p, w).view(np.int32), p.view(np.int32))
    got[7] = np.nan
    assert EC.outside(got, e, p, w)[0] == 1


def test_accumulated_bound_covers_the_emulation():
    e0, _ = _data(4099, 9)
    r = np.random.default_rng(11)
    ws = [ema_weight(0.9, u, True) for u in range(1, 5)]
    ps, es, e = [], [], e0
    for w in ws:
        p = (e + 3e-3 * r.standard_normal(e.size)).astype(np.float32)
        ps.append(p)
        es.append(e)
        e = EC.emulate(e, p, w)
    B = EC.accumulated_bound(es, ps, ws)
    assert (np.abs(e.astype(np.float64) - EC.recurrence(e0, ps, ws)) <= B).all()
    assert (B <= 4 * EC.bound(e, ps[-1], 1.0)).all()  # four updates: no more than four single-update bounds at full weight


def test_ema_weight_schedule():
    for d in (0.9, 0.999, 0.5):
        for u in (1, 2, 17, 10_000):
            assert ema_weight(d, u, False) == 1.0 - d == EC.weight(d, u, False)
            assert ema_weight(d, u) == 1.0 - d
    d = 0.999
    assert [ema_weight(d, u, True) for u in (1, 2, 3)] == [1 - 2 / 11, 1 - 3 / 12, 1 - 4 / 13]
    for u in range(1, 20_000, 7):
        want = 1.0 - min(d, (1.0 + u) / (10.0 + u))
        assert ema_weight(d, u, True) == want == EC.weight(d, u, True)
        assert 1.0 - d <= ema_weight(d, u, True) <= 1.0 - 2 / 11
    # (1 + u) / (10 + u) reaches 0.999 at u = 8990 (there the two are equal up to the rounding of the quotient)
    assert ema_weight(d, 8989, True) > 1.0 - d and ema_weight(d, 8991, True) == 1.0 - d
    assert ema_weight(0.1, 1, True) == 1.0 - 0.1  # a decay below 2/11 is the cap from the first update
    with pytest.raises(ValueError):
        ema_weight(0.9, 0)
