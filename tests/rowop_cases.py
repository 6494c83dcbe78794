"""The case table of the row-op kernels (frozenbilm_amd/csrc/rowops.hip), shared by the CPU test of the table itself
(tests/test_rowop_cases.py) and the GPU tests that run every case against fp64 (tests/test_gpu_rowops.py).

Each case names one call of an entry point -- shape, options -- and the branch of the launcher / kernel it is there for.
The caps the branches depend on are not written down here: they come from the library's own host queries (no GPU needed)

    LNB_BLOCKS   = fbl_ln_bwd_ws_floats(H) // (3 * H)     persistent grid of fbl_ln_bwd
    CS_BLOCKS    = fbl_colsum_ws_floats(cols) // cols     row blocks of fbl_colsum
    SUMSQ_BLOCKS = fbl_sumsq_ws_floats()                  partial sums of fbl_sumsq

so a change of a cap moves the cases that are defined relative to it, and tests/test_rowop_cases.py says which of the
remaining ones stopped covering their branch.  The helpers below restate, from the launchers, what decides a branch.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

# grid1d() of rowops.hip ("inline int grid1d(long n, int block = 256, int cap = 256 * 16)"): the element-wise kernels run at
# most GRID1D_CAP blocks of GRID1D_BLOCK threads and stride over the rest.  There is no host query for it; the big element-wise
# cases are more than 4x larger so that a moderate change of the cap keeps them on the grid-stride loop.
GRID1D_BLOCK, GRID1D_CAP = 256, 256 * 16
BIG_N = 5 * GRID1D_BLOCK * GRID1D_CAP + 3

LN_HS = (64, 128, 256, 512, 768, 1024, 1536, 2048)  # every FBL_EPL_DISPATCH instantiation (H / 64 in 1 2 4 8 12 16 24 32)
FOLD_DEEP = 224        # ln_bwd_fold_kernel: the eight-loads-in-flight loop runs while b + 224 < nblk
CE_FOLD_THREADS = 256  # ce_fold_kernel: thread t takes rows t, t + 256, ...
VOCAB = 128100         # deberta-v2-xlarge


@dataclass(frozen=True)
class Caps:
    LNB_BLOCKS: int
    CS_BLOCKS: int
    SUMSQ_BLOCKS: int


@lru_cache(maxsize=None)
def caps() -> Caps:
    """the caps, asked of the library itself (built first if it is not there yet; plain host calls)"""
    from frozenbilm_amd import lib

    if os.path.exists(lib.LIB_PATH):
        h = lib.load()
    else:
        from frozenbilm_amd.build import build_lib

        h = lib.load(build_lib(verbose=False))
    lnb = {h.fbl_ln_bwd_ws_floats(H) // (3 * H) for H in LN_HS}
    cs = {h.fbl_colsum_ws_floats(c) // c for c in (16, 200, 1536)}
    assert len(lnb) == 1 and len(cs) == 1, (lnb, cs)
    return Caps(lnb.pop(), cs.pop(), int(h.fbl_sumsq_ws_floats()))


# ------------------------------------------------------------------------------------------------ what decides a branch
def ln_bwd_kernel(H: int) -> str:
    """fbl_ln_bwd: even H/64 -> ln_bwd2_kernel (two waves per row, two rows per block iteration), odd -> ln_bwd_kernel"""
    return "ln_bwd2" if (H // 64) % 2 == 0 else "ln_bwd"


def ln_bwd_rows_per_block(H: int) -> int:
    return 2 if ln_bwd_kernel(H) == "ln_bwd2" else 4


def ln_bwd_want_blocks(N: int, H: int) -> int:
    r = ln_bwd_rows_per_block(H)
    return (N + r - 1) // r


def ln_bwd_nblk(N: int, H: int, cap: int) -> int:
    """blocks launched = partial rows the fold reads"""
    return min(ln_bwd_want_blocks(N, H), cap)


def ln_bwd_iters(N: int, H: int, cap: int) -> int:
    """loop iterations of block 0 (the most any block does)"""
    nb = ln_bwd_nblk(N, H, cap)
    return (ln_bwd_want_blocks(N, H) + nb - 1) // nb


def ln_bwd_dead_slot_iter(N: int, H: int, cap: int) -> Optional[int]:
    """ln_bwd2_kernel with odd N: the 0-based iteration in which some block meets `live == false`, else None"""
    if ln_bwd_kernel(H) != "ln_bwd2" or N % 2 == 0:
        return None
    return ((N - 1) // 2) // ln_bwd_nblk(N, H, cap)


def sumsq_nblk(n: int, cap: int) -> int:
    return max(1, min((n + GRID1D_BLOCK - 1) // GRID1D_BLOCK, cap))


# ------------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class LnFwd:
    name: str
    H: int
    N: int
    y: Optional[str] = "full"          # None | "full" | "slice" (a column slice of a wider buffer: ldy > H)
    r_plain: bool = False
    r_norm: Optional[str] = None       # None | "plain" | "masked" (r_norm with its own row mask)
    rowmask: bool = False
    p: float = 0.0
    outs: Tuple[str, ...] = ("f32",)   # of "bf16", "f32"
    why: str = ""


@dataclass(frozen=True)
class LnMat:
    name: str
    H: int
    N: int
    rowmask: bool = False
    add_bcast: int = 0                 # S of the broadcast add (0: none)
    outs: Tuple[str, ...] = ("f32", "bf16")
    why: str = ""


@dataclass(frozen=True)
class LnBwd:
    name: str
    H: int
    N: int
    rowmask: bool = False
    p: float = 0.0
    out_dt: bool = True
    dy: Tuple[str, ...] = ()           # of "bf16" (ld = H), "bf16_wide" (inside a wider buffer), "f32"
    fold: Tuple[str, ...] = ("dgamma", "dbeta", "dysum")
    int_dout: bool = False             # integer dout: dbeta must be exact
    twice: bool = False                # run twice with a different ws prefill: dgamma / dbeta / dysum bit-identical
    why: str = ""


@dataclass(frozen=True)
class Ce:
    name: str
    N: int
    V: int
    ld: int
    gscale: str = "float"              # "float" | "tensor"
    rows: str = "labelled"             # "labelled" | "padded" (ignored entries + repeated padding in a fixed-capacity list)
    twice: bool = False
    why: str = ""

    @property
    def Vp(self):
        return (self.V + 63) // 64 * 64


@dataclass(frozen=True)
class SumSq:
    name: str
    n: int
    exact: bool
    twice: bool = False
    why: str = ""


@dataclass(frozen=True)
class Adam:
    name: str
    n: int
    wd: float = 0.0
    grad_scale: float = 1.0
    max_norm: str = "none"             # "none" (0) | "below" (max_norm < norm: clipped) | "above" (max_norm > norm: not clipped)
    steps: Tuple[int, ...] = (1, 2, 3)
    why: str = ""


@dataclass(frozen=True)
class ColSum:
    name: str
    rows: int
    cols: int
    bf16: bool = False
    width: Optional[int] = None        # columns of the tensor (cols < width: only the first cols are summed)
    ld: Optional[int] = None           # row stride of the input
    twice: bool = False
    why: str = ""


@dataclass(frozen=True)
class Elem:
    name: str
    op: str                            # gelu_fwd | gelu_bwd | dropout_f32 | dropout_bf16 | cast
    n: int
    p: float = 0.0
    why: str = ""


@dataclass(frozen=True)
class RowsCase:
    name: str
    op: str                            # gather | scatter
    cols: int
    R: int
    src_rows: int
    repeated: bool = False
    why: str = ""


PROD_N, PROD_H = 8512, 1536  # rows and hidden size of a training step


def ln_fwd_cases():
    out = []
    for H in LN_HS:
        for N in (1, 3, 203):
            out.append(LnFwd(f"fwd_H{H}_N{N}", H, N, r_plain=True, rowmask=N > 1, outs=("bf16", "f32"),
                             why="EPL instantiation; N not a multiple of 4"))
    out += [
        LnFwd("fwd_prod", PROD_H, PROD_N, r_plain=True, rowmask=True, p=0.1, outs=("bf16",), why="production shape, dropout live"),
        LnFwd("fwd_opt_y_only", 1024, 203, why="no residual"),
        LnFwd("fwd_opt_y_none", 768, 203, y=None, r_plain=True, why="y = None"),
        LnFwd("fwd_opt_y_slice", 1536, 203, y="slice", r_plain=True, p=0.1, outs=("bf16", "f32"), why="ldy > H, dropout keyed by m*H + n"),
        LnFwd("fwd_opt_rnorm", 2048, 203, r_norm="plain", outs=("bf16",), why="r_norm without a row mask, large H"),
        LnFwd("fwd_opt_rnorm_masked", 2048, 203, r_norm="masked", rowmask=True, outs=("f32",), why="r_norm with its own row mask, large H"),
        LnFwd("fwd_opt_rnorm_plain_both", 512, 203, r_plain=True, r_norm="masked", p=0.1, outs=("bf16", "f32"), why="all three addends"),
        LnFwd("fwd_opt_p01_H64", 64, 203, p=0.1, rowmask=True, outs=("f32",), why="dropout at VEC = 1"),
        LnFwd("fwd_opt_no_out", 256, 203, r_plain=True, outs=(), why="statistics and t only"),
    ]
    return out


def ln_mat_cases():
    out = []
    for H in LN_HS:
        for N in (1, 3, 203):
            out.append(LnMat(f"mat_H{H}_N{N}", H, N, rowmask=N > 1, add_bcast=7 if N == 203 else 0,
                             why="EPL instantiation; N not a multiple of 4"))
    out.append(LnMat("mat_prod", PROD_H, PROD_N, rowmask=True, outs=("bf16",), why="production shape"))
    out.append(LnMat("mat_f32_only", 1024, 203, add_bcast=5, outs=("f32",), why="fp32 output alone"))
    return out


def ln_bwd_cases():
    c = caps()
    cap = c.LNB_BLOCKS
    out = []
    for H in LN_HS:
        for N in (1, 2, 3, 203):
            out.append(LnBwd(f"bwd_H{H}_N{N}", H, N, rowmask=N > 2, dy=("bf16",), int_dout=(N == 203),
                             why="EPL instantiation of ln_bwd2 / ln_bwd; one iteration; fold's scalar tail"))
    # relative to the cap (ln_bwd2: two rows per block iteration)
    out += [
        LnBwd("bwd_at_cap_minus", 256, 2 * cap - 1, rowmask=True, dy=("f32",), why="nblk == cap, one iteration, dead slot in it"),
        LnBwd("bwd_over_cap", 512, 2 * cap + 1, rowmask=True, dy=("bf16",), why="second iteration holds one row and no dead slot"),
        LnBwd("bwd_over_cap_dead", 1024, 2 * cap + 3, dy=("bf16",), int_dout=True, why="dead slot in the second iteration"),
        LnBwd("bwd_H64_iters", 64, 4 * cap + 3, rowmask=True, dy=("f32",), int_dout=True,
              why="ln_bwd_kernel (odd H/64): second iteration with three live waves"),
        LnBwd("bwd_H64_many", 64, 12 * cap + 5, rowmask=True, dy=("bf16",), why="ln_bwd_kernel: four iterations"),
        LnBwd("bwd_N8512_H1024", 1024, PROD_N, rowmask=True, p=0.1, dy=("bf16",), why="bert-large hidden size, several iterations"),
        LnBwd("bwd_N8513_H2048", 2048, PROD_N + 1, rowmask=True, dy=("bf16",), int_dout=True,
              why="odd N: the dead slot falls in the last of several iterations"),
        LnBwd("bwd_N8513_H128", 128, PROD_N + 1, dy=("f32",), p=0.1, why="odd N, several iterations, VEC = 1 of ln_bwd2"),
        LnBwd("bwd_N8512_H768", 768, PROD_N, rowmask=True, dy=("bf16",), int_dout=True, why="bert-base hidden size, VEC = 2"),
        # the option combinations engine._ln_bwd uses
        LnBwd("bwd_prod_full", PROD_H, PROD_N, rowmask=True, p=0.1, dy=("bf16_wide",), twice=True,
              why="rowmask + dropout + dy inside the [dy | dz] operand + dysum + out_dt"),
        LnBwd("bwd_prod_8513", PROD_H, PROD_N + 1, rowmask=True, p=0.1, dy=("bf16_wide", "f32"), int_dout=True,
              why="production options at odd N"),
        LnBwd("bwd_opt_dgamma_dbeta", PROD_H, PROD_N, rowmask=True, dy=(), fold=("dgamma", "dbeta"), int_dout=True,
              why="only dgamma / dbeta (the head's LayerNorm: want_dy_bf16 = False, no dysum)"),
        LnBwd("bwd_opt_no_fold", PROD_H, 1001, p=0.1, dy=("bf16",), fold=(), why="no fold outputs at all"),
        LnBwd("bwd_opt_no_dt", 512, 203, out_dt=False, dy=("bf16", "f32"), fold=("dysum",), why="dy without dt; dysum alone"),
    ]
    return out


def ce_cases():
    return [
        Ce("ce_small_vec", 37, 1003, 1024, rows="padded", why="vector loads, tail of V % 4"),
        Ce("ce_small_scalar", 37, 1003, 1003, gscale="tensor", why="ldv % 4 != 0: scalar path"),
        Ce("ce_vocab", 700, VOCAB, (VOCAB + 63) // 64 * 64, gscale="tensor", rows="padded", twice=True,
           why="production vocabulary, fold over > 256 rows"),
        Ce("ce_mid", 1000, 4099, 4160, why="V % 4 == 3, fold with four rows per thread"),
    ]


def sumsq_cases():
    c = caps()
    at_cap = GRID1D_BLOCK * c.SUMSQ_BLOCKS
    return [
        SumSq("ss_1", 1, True, why="one block, one element"),
        SumSq("ss_255", 255, True, why="one block, not full"),
        SumSq("ss_10007", 10007, True, why="40 blocks"),
        SumSq("ss_at_cap", at_cap, True, why="exactly SUMSQ_BLOCKS blocks, one element per thread"),
        SumSq("ss_over_cap", at_cap + 1, True, why="grid-stride: one thread takes two elements; full-width fold"),
        SumSq("ss_big_exact", 3 * at_cap + 77, True, why="several elements per thread, still exact (16 n < 2^24)"),
        SumSq("ss_big", BIG_N, False, twice=True, why="largest: 20 elements per thread"),
    ]


def adam_cases():
    c = caps()
    return [
        Adam("adam_1", 1, wd=0.01, max_norm="below", why="one element"),
        Adam("adam_255", 255, grad_scale=1 / 8, max_norm="above", why="un-clipped branch"),
        Adam("adam_10007", 10007, max_norm="below", why="the shape of test_adam_and_sumsq"),
        Adam("adam_10007_wd", 10007, wd=0.01, grad_scale=1 / 8, max_norm="below", why="weight decay, grad_scale, clipped"),
        Adam("adam_ss_cap", GRID1D_BLOCK * c.SUMSQ_BLOCKS + 1, wd=0.01, max_norm="above", why="sumsq over its cap feeding the clip"),
        Adam("adam_big", BIG_N, wd=0.01, grad_scale=1 / 8, max_norm="below", steps=(1, 2), why="both grid-stride loops"),
        Adam("adam_step1000", 10007, wd=0.01, max_norm="none", steps=(1000,), why="bias corrections near 1; no clipping"),
    ]


def colsum_cases():
    c = caps()
    return [
        ColSum("cs_333x200", 333, 200, why="one row per block"),
        ColSum("cs_333x200_bf16_part", 333, 100, bf16=True, width=200, why="cols < width"),
        ColSum("cs_8512x192", PROD_N, 192, bf16=True, ld=192 + 1536, why="production adapter bias gradient, ld_in > cols"),
        ColSum("cs_8512x1536", PROD_N, 1536, twice=True, why="production, blockIdx.y up to 5, grid-stride over rows"),
        ColSum("cs_8512x1536_bf16", PROD_N, 1536, bf16=True, why="production, bf16 input"),
        ColSum("cs_over_cap", c.CS_BLOCKS + 1, 257, ld=264, why="block 0 takes two rows; the last column slab holds one column"),
        ColSum("cs_1x16", 1, 16, why="one row, one fold block"),
        ColSum("cs_17x16_bf16", 17, 16, bf16=True, ld=24, why="fold16 comes round once (nblk = 17 > 16)"),
    ]


def elem_cases():
    out = []
    for op in ("gelu_fwd", "gelu_bwd", "dropout_f32", "dropout_bf16"):
        for n, p in ((1, 0.25), (5000, 0.0), (5000, 0.1), (5000, 0.25), (BIG_N, 0.1)):
            if op == "dropout_bf16" and p == 0.0:
                continue  # (fbl_dropout_bf16 with p = 0 is a no-op by contract: checked in the p > 0 test body)
            out.append(Elem(f"{op}_n{n}_p{p}", op, n, p, why="grid-stride" if n == BIG_N else "values under dropout"))
    for n in (1, 5000, BIG_N):
        out.append(Elem(f"cast_n{n}", "cast", n, why="grid-stride" if n == BIG_N else "RNE, ties, denormals"))
    return out


def rows_cases():
    return [
        RowsCase("gather_64", "gather", 64, 700, 1000, repeated=True, why="one pass of the column loop"),
        RowsCase("gather_1536", "gather", 1536, 700, 1000, repeated=True, why="more than 128 threads x 8 columns"),
        RowsCase("scatter_64", "scatter", 64, 700, 1000, why="one pass"),
        RowsCase("scatter_1536", "scatter", 1536, 700, 1000, why="six passes of the column loop"),
    ]


def ids(cases):
    return [c.name for c in cases]
