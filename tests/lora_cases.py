"""The cases of the LoRA compose kernel (include/fbl_lora.h), their float64 reference and the judge, in numpy only: shared by
tests/test_lora_cases.py (CPU: the reference against a second statement, the share of elements near a rounding boundary) and
tests/test_gpu_lora_compose.py (the kernel against the reference).

    W' = W + s . B . A        W [O, I], A [r, I], B [O, r]   ->   bf16, round to nearest even, once

The judge: the kernel accumulates in fp32 (r fused multiply-adds, then one fused multiply-add with s and W), so its fp32 value v
satisfies |v - x| <= (r + 2) . 2^-24 . (|W| + |s| . sum_k |B||A|) of the float64 value x (the standard bound of a length-r dot
product in a format with unit round-off 2^-24, plus the two last operations; derived, not tuned).  bf16(v) can differ from
bf16(x) only when x lies within that bound of a bf16 rounding boundary -- the midpoint of two neighbouring bf16 values -- and
then it is the value on the other side of that boundary.
"""
import numpy as np

# (O, I, r): one tile and rank 1; two row tiles; a non-square site at the largest rank; the true widths of the model
CASES = [(64, 64, 1), (128, 64, 8), (192, 128, 64), (1536, 1536, 16)]
SCALE = 2.0  # alpha = 2 r, the common choice
U = 2.0 ** -24


def inputs(O, I, r, seed=0, scale=None):
    """W ~ N(0, 0.02) like a trained projection, A ~ U(+-1/sqrt(I)) (nn.Linear's initialisation), B ~ N(0, 0.02 / sqrt(r)); fp32.
    B shrinks with the rank so that the update s.B.A stays of the size of W at every r: the judge's bound grows with
    |s| . sum |B||A|, and an update that dwarfs W would put more than 1 % of the elements into the boundary band by the
    reference alone (tests/test_lora_cases.py checks the share).  Two rows of B are zero (a LoRA row that never trained):
    their result is exactly bf16(W)."""
    g = np.random.default_rng(1000 * r + O + I + seed)
    W = (g.standard_normal((O, I)) * 0.02).astype(np.float32)
    A = ((g.random((r, I)) * 2 - 1) / np.sqrt(I)).astype(np.float32)
    B = (g.standard_normal((O, r)) * (0.02 / np.sqrt(r))).astype(np.float32)
    B[3] = 0
    B[O - 1] = 0
    # Where W and s.B.A cancel almost completely the fp32 bound exceeds the spacing of the bf16 values around x: the float64
    # value then pins no single neighbour and the judge below would be ill-posed (one element in two million at the true
    # widths).  Such elements get a W that does not cancel -- a property of the reference alone, checked by
    # tests/test_lora_cases.py for every element: bound < ulp / 8.
    x, bound = reference(W, A, B, SCALE if scale is None else scale)  # (the scale the case is run at)
    ulp = np.ldexp(1.0, np.frexp(x)[1] - 8)
    W[bound >= ulp / 8] += np.float32(0.01)
    return W, A, B


def reference(W, A, B, s):
    """(x, bound): the float64 value of W + s.B.A and the fp32 accumulation bound of the module docstring, per element"""
    W64, A64, B64 = W.astype(np.float64), A.astype(np.float64), B.astype(np.float64)
    x = W64 + float(s) * (B64 @ A64)
    mag = np.abs(W64) + abs(float(s)) * (np.abs(B64) @ np.abs(A64))
    return x, (A.shape[0] + 2) * U * mag


def bf16_grid(x):
    """(rne, lo, hi, mid) float64 arrays: bf16(x) rounded to nearest even, the bf16 neighbours lo <= x < hi (lo = x when x is a
    bf16 value) and their midpoint.  Normal range only (the cases stay far from the subnormals)."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)                      # x = m . 2^e, 0.5 <= |m| < 1: 8 significant bits = m . 2^8
    ulp = np.ldexp(1.0, e - 8)
    rne = np.rint(m * 256.0) * ulp          # (np.rint rounds halves to even)
    lo = np.floor(m * 256.0) * ulp
    hi = lo + ulp
    return rne, lo, hi, lo + 0.5 * ulp


def in_band(x, bound):
    """elements whose float64 value lies within `bound` of a bf16 rounding boundary"""
    _, _, _, mid = bf16_grid(x)
    return np.abs(np.asarray(x, dtype=np.float64) - mid) <= bound


def bf16_bits_to_f64(bits):
    """uint16 / int16 bf16 bit patterns -> their values (exact)"""
    b = np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16
    return b.view(np.float32).astype(np.float64)


def judge(got, x, bound):
    """got: the kernel's bf16 results as float64 values.  Returns (wrong, n_band): a boolean array of the elements that break
    the rule of the module docstring, and how many elements lie in the boundary band."""
    rne, lo, hi, _ = bf16_grid(x)
    band = in_band(x, bound)
    ok = (got == rne) | (band & ((got == lo) | (got == hi)))
    return ~ok, int(band.sum())
