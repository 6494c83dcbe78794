"""CPU: the case table of the LoRA compose kernel (tests/lora_cases.py) -- its float64 reference against a second, plain
statement; its bf16 grid against torch's own rounding; and the share of elements the reference ALONE leaves near a rounding
boundary (at most 1 %: the GPU judge is exact everywhere else)."""
import numpy as np
import pytest
import torch

from tests import lora_cases as LC


@pytest.mark.parametrize("O,I,r", LC.CASES[:3])
def test_reference_equals_the_elementwise_statement(O, I, r):
    W, A, B = LC.inputs(O, I, r)
    x, bound = LC.reference(W, A, B, LC.SCALE)
    g = np.random.default_rng(5)
    for o, i in zip(g.integers(0, O, 200), g.integers(0, I, 200)):
        acc, mag = 0.0, 0.0
        for k in range(r):
            acc += float(B[o, k]) * float(A[k, i])
            mag += abs(float(B[o, k])) * abs(float(A[k, i]))
        want = float(W[o, i]) + LC.SCALE * acc
        assert abs(x[o, i] - want) <= 1e-15 * (abs(want) + 1e-30) * (r + 2), (o, i)
        assert abs(bound[o, i] - (r + 2) * 2.0 ** -24 * (abs(float(W[o, i])) + LC.SCALE * mag)) <= 1e-12 * bound[o, i]
    assert np.array_equal(x[3], W[3].astype(np.float64)) and np.array_equal(x[O - 1], W[O - 1].astype(np.float64))  # zero rows of B


def test_bf16_grid_is_torch_rounding():
    g = np.random.default_rng(9)
    x = np.concatenate([g.standard_normal(20000) * 0.05, [1.0, -1.0, 0.5, 1.00390625, 1.01171875, -0.01953125, 0.0]])
    x32 = x.astype(np.float32).astype(np.float64)  # values a float holds exactly: torch's float -> bf16 is then one rounding
    rne, lo, hi, mid = LC.bf16_grid(x32)
    want = torch.from_numpy(x32.astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(rne, want)
    assert np.all(lo <= x32) and np.all(x32 < hi) and np.all((rne == lo) | (rne == hi))
    bits = torch.from_numpy(x32.astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy()
    assert np.array_equal(LC.bf16_bits_to_f64(bits), want)
    # exact halves go to the even neighbour: 1 + 2^-8 is the midpoint of 1 and 1 + 2^-7
    assert LC.bf16_grid(np.array([1.00390625]))[0][0] == 1.0 and LC.bf16_grid(np.array([1.01171875]))[0][0] == 1.015625


@pytest.mark.parametrize("O,I,r", LC.CASES)
def test_at_most_one_percent_of_the_elements_lie_in_the_boundary_band(O, I, r):
    W, A, B = LC.inputs(O, I, r)
    x, bound = LC.reference(W, A, B, LC.SCALE)
    ulp = np.ldexp(1.0, np.frexp(x)[1] - 8)
    assert (bound < ulp / 8).all(), "an element cancels so far that the fp32 bound spans several bf16 values"
    share = LC.in_band(x, bound).mean()
    print(f"(O, I, r) = {(O, I, r)}: {100 * share:.3f} % of the elements within the fp32 bound of a bf16 boundary")
    assert share <= 0.01


def test_judge_accepts_the_reference_and_refuses_a_wrong_neighbour():
    O, I, r = LC.CASES[1]
    W, A, B = LC.inputs(O, I, r)
    x, bound = LC.reference(W, A, B, LC.SCALE)
    rne, lo, hi, _ = LC.bf16_grid(x)
    wrong, _ = LC.judge(rne, x, bound)
    assert not wrong.any()
    far = ~LC.in_band(x, bound)
    other = np.where(rne == lo, hi, lo)
    wrong, _ = LC.judge(other, x, bound)
    assert wrong[far].all()          # outside the band only bf16(x) passes
    assert not wrong[~far].any()     # inside it, the value across the boundary passes too ...
    wrong, _ = LC.judge(hi + (hi - lo), x, bound)
    assert wrong.all()               # ... and nothing further away
