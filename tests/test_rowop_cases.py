"""CPU: the row-op case table (tests/rowop_cases.py) really covers the branches it claims to, judged from the caps the library
reports (fbl_ln_bwd_ws_floats, fbl_colsum_ws_floats, fbl_sumsq_ws_floats: host queries, no HIP call), and the argument errors
the launchers of rowops.hip return before any HIP call.

If LNB_BLOCKS, CS_BLOCKS or SUMSQ_BLOCKS change, the cases defined relative to them move along; a failure here names the
branch that a fixed-size case no longer reaches."""
import ctypes as C

import pytest

from tests import rowop_cases as RC

ERR_SHAPE, ERR_ALIGN, ERR_ARG = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib
    from frozenbilm_amd.build import build_lib

    lib.load(build_lib(verbose=False))
    return lib


@pytest.fixture(scope="module")
def caps(L):
    return RC.caps()


def test_caps_are_the_library_s(L, caps):
    h = L.load()
    assert caps.LNB_BLOCKS == h.fbl_ln_bwd_ws_floats(1536) // (3 * 1536) > 0
    assert caps.CS_BLOCKS == h.fbl_colsum_ws_floats(192) // 192 > 0
    assert caps.SUMSQ_BLOCKS == h.fbl_sumsq_ws_floats() > 0


def test_case_names_are_unique(caps):
    for cases in (RC.ln_fwd_cases(), RC.ln_mat_cases(), RC.ln_bwd_cases(), RC.ce_cases(), RC.sumsq_cases(), RC.adam_cases(),
                  RC.colsum_cases(), RC.elem_cases(), RC.rows_cases()):
        names = RC.ids(cases)
        assert len(set(names)) == len(names), names


def test_every_ln_instantiation_on_each_of_the_four_kernels(caps):
    fwd = {c.H for c in RC.ln_fwd_cases()}
    mat = {c.H for c in RC.ln_mat_cases()}
    bwd = {c.H for c in RC.ln_bwd_cases()}
    for H in RC.LN_HS:
        assert H in fwd, f"ln_fwd_kernel<{H // 64}> has no case"
        assert H in mat, f"ln_mat_kernel<{H // 64}> has no case"
        assert H in bwd, f"{RC.ln_bwd_kernel(H)}_kernel<{H // 64}> has no case"
    kernels = {RC.ln_bwd_kernel(c.H) for c in RC.ln_bwd_cases()}
    assert kernels == {"ln_bwd", "ln_bwd2"}, f"LayerNorm backward kernels without a case: {kernels ^ {'ln_bwd', 'ln_bwd2'}}"
    assert any((c.H // 64) % 2 == 1 for c in RC.ln_bwd_cases()), "no ln_bwd case with odd H/64 (ln_bwd_kernel)"
    # rows that are not a multiple of the 4 rows a forward block holds, and the production shape
    for cases, what in ((RC.ln_fwd_cases(), "ln_fwd"), (RC.ln_mat_cases(), "ln_materialize")):
        assert {1, 3, 203} <= {c.N for c in cases}, what
        assert any((c.N, c.H) == (RC.PROD_N, RC.PROD_H) for c in cases), f"{what}: no production shape"


def test_ln_fwd_options(caps):
    cs = RC.ln_fwd_cases()
    assert any(c.y is None for c in cs), "y = None"
    assert any(c.y == "slice" for c in cs), "y as a column slice (ldy > H)"
    assert any(c.y == "slice" and c.p > 0 for c in cs), "dropout keyed by m*H + n (not m*ldy + n) is only visible with ldy > H"
    assert any(c.r_plain for c in cs) and any(not c.r_plain for c in cs)
    assert any(c.r_norm == "plain" for c in cs) and any(c.r_norm == "masked" for c in cs)
    assert any(c.r_norm and c.H >= 1536 for c in cs), "r_norm at a large H"
    assert any(c.rowmask for c in cs) and any(not c.rowmask for c in cs)
    assert {0.0, 0.1} <= {c.p for c in cs}
    assert {("bf16",), ("f32",), ("bf16", "f32")} <= {c.outs for c in cs}


def test_ln_bwd_loop_and_fold_branches(caps):
    cap = caps.LNB_BLOCKS
    cs = RC.ln_bwd_cases()
    for k in ("ln_bwd", "ln_bwd2"):
        mine = [c for c in cs if RC.ln_bwd_kernel(c.H) == k]
        assert any(RC.ln_bwd_want_blocks(c.N, c.H) < cap for c in mine), f"{k}: no case with nblk < LNB_BLOCKS ({cap})"
        assert any(RC.ln_bwd_iters(c.N, c.H, cap) >= 2 for c in mine), f"{k}: the grid-stride row loop never comes round"
        assert any(RC.ln_bwd_iters(c.N, c.H, cap) >= 3 for c in mine), \
            f"{k}: no case with at least 3 loop iterations per block at LNB_BLOCKS = {cap}"
    two = [c for c in cs if RC.ln_bwd_kernel(c.H) == "ln_bwd2"]
    assert any(RC.ln_bwd_want_blocks(c.N, c.H) == cap for c in two), f"ln_bwd2: no case with nblk == LNB_BLOCKS ({cap}) exactly"
    assert any(RC.ln_bwd_want_blocks(c.N, c.H) == cap + 1 for c in two), "ln_bwd2: no case one block over the cap"
    # the parity double buffer of xch needs three iterations to reuse a slot
    assert any(RC.ln_bwd_iters(c.N, c.H, cap) >= 3 and c.H == RC.PROD_H for c in two), "production H does not reuse an xch slot"
    # odd N: the dead slot in the first, in a later, and in the last of >= 3 iterations
    dead = [(RC.ln_bwd_dead_slot_iter(c.N, c.H, cap), RC.ln_bwd_iters(c.N, c.H, cap)) for c in two]
    dead = [(d, it) for d, it in dead if d is not None]
    assert any(d == 0 for d, it in dead), "ln_bwd2: no odd N whose dead slot is in the first iteration"
    assert any(d >= 1 for d, it in dead), "ln_bwd2: no odd N whose dead slot is in a later iteration"
    assert any(d == it - 1 and it >= 3 for d, it in dead), "ln_bwd2: no odd N whose dead slot is in the last of >= 3 iterations"
    # ln_bwd_kernel: a last iteration in which only some of the four waves have a row
    one = [c for c in cs if RC.ln_bwd_kernel(c.H) == "ln_bwd"]
    assert any(RC.ln_bwd_iters(c.N, c.H, cap) >= 2 and c.N % 4 for c in one), "ln_bwd: no ragged later iteration"
    # the fold: scalar tail only / the eight-deep loop
    folded = [c for c in cs if c.fold]
    assert any(RC.ln_bwd_nblk(c.N, c.H, cap) <= RC.FOLD_DEEP for c in folded), "ln_bwd_fold: no case with nblk <= 224"
    assert any(RC.ln_bwd_nblk(c.N, c.H, cap) > RC.FOLD_DEEP for c in folded), \
        f"ln_bwd_fold: the eight-loads-in-flight loop needs nblk > {RC.FOLD_DEEP} partial rows; no case has them at LNB_BLOCKS = {cap}"


def test_ln_bwd_options(caps):
    cs = RC.ln_bwd_cases()
    assert any(c.rowmask and c.p > 0 and "bf16_wide" in c.dy and "dysum" in c.fold and c.out_dt and (c.N, c.H) == (RC.PROD_N, RC.PROD_H)
               for c in cs), "the full option set of engine._ln_bwd at the production shape"
    assert any(set(c.fold) == {"dgamma", "dbeta"} for c in cs), "only dgamma / dbeta"
    assert any(not c.fold for c in cs), "no fold outputs at all"
    assert any(not c.out_dt for c in cs) and any("f32" in c.dy for c in cs) and any(not c.dy for c in cs)
    assert any(c.int_dout and c.rowmask and "dbeta" in c.fold and RC.ln_bwd_iters(c.N, c.H, caps.LNB_BLOCKS) >= 3 for c in cs), \
        "exact dbeta over several iterations"
    assert {1, 2, 3, 203, RC.PROD_N, RC.PROD_N + 1} <= {c.N for c in cs}


def test_ce_branches(caps):
    cs = RC.ce_cases()
    assert any(c.ld % 4 != 0 for c in cs), "no CE case with ldv % 4 != 0 (scalar loads)"
    assert any(c.ld % 4 == 0 and c.V % 4 != 0 for c in cs), "no CE case with vector loads and a tail of V % 4"
    assert any(c.N > RC.CE_FOLD_THREADS for c in cs), "ce_fold_kernel: no case with more rows than threads"
    assert any(c.N > 3 * RC.CE_FOLD_THREADS for c in cs), "ce_fold_kernel: no case with several rows per thread"
    assert any(c.V == RC.VOCAB and c.ld == (RC.VOCAB + 63) // 64 * 64 for c in cs), "production vocabulary at the engine's ldv"
    assert {"float", "tensor"} == {c.gscale for c in cs}
    assert any(c.rows == "padded" for c in cs), "row list with ignored entries and repeated padding"
    assert all(c.ld >= c.V for c in cs)


def test_sumsq_and_adam_branches(caps):
    cap = caps.SUMSQ_BLOCKS
    ss = RC.sumsq_cases()
    assert any(RC.sumsq_nblk(c.n, cap) == 1 for c in ss), "sumsq: no one-block case"
    assert any(c.n == RC.GRID1D_BLOCK * cap for c in ss), "sumsq: no case with exactly SUMSQ_BLOCKS full blocks"
    assert any(c.n > RC.GRID1D_BLOCK * cap for c in ss), "sumsq: no case with more than one element per thread"
    assert any(RC.sumsq_nblk(c.n, cap) == cap > 256 for c in ss) or cap <= 256, "sumsq_fold: no full-width fold"
    for c in ss:
        assert (not c.exact) or c.n * 16 < 2 ** 24, f"{c.name}: integers in [-4, 4] are not exact in fp32 at this n"
    assert any(not c.exact and c.n > 4 * RC.GRID1D_BLOCK * RC.GRID1D_CAP for c in ss)
    ad = RC.adam_cases()
    assert {0.0, 0.01} <= {c.wd for c in ad} and {1.0, 1 / 8} <= {c.grad_scale for c in ad}
    assert {"none", "below", "above"} == {c.max_norm for c in ad}
    assert any(c.steps == (1, 2, 3) for c in ad) and any(c.steps == (1000,) for c in ad)
    assert any(c.n > 4 * RC.GRID1D_BLOCK * RC.GRID1D_CAP for c in ad), "adam_flat: no case on the grid-stride loop"
    assert {1, 255, 10007, RC.GRID1D_BLOCK * cap + 1, RC.BIG_N} <= {c.n for c in ad} | {c.n for c in ss}


def test_colsum_branches(caps):
    cap = caps.CS_BLOCKS
    cs = RC.colsum_cases()
    assert any(c.rows > cap for c in cs), f"colsum: no case with rows > CS_BLOCKS ({cap})"
    assert any(c.rows > 2 * cap for c in cs), "colsum: no case with several rows per block"
    assert any(c.rows < cap for c in cs)
    assert any(c.cols > 256 for c in cs), "colsum: blockIdx.y is always 0"
    assert any(c.cols % 256 for c in cs if c.cols > 256), "colsum: no ragged last column slab"
    assert any(min(c.rows, cap) > 16 for c in cs), "fold16 never comes round"
    assert any(c.bf16 for c in cs) and any(not c.bf16 for c in cs)
    assert any(c.width and c.width > c.cols for c in cs) and any(c.ld and c.ld > c.cols for c in cs)
    assert {(333, 200), (RC.PROD_N, 192), (RC.PROD_N, 1536), (cap + 1, 257), (1, 16)} <= {(c.rows, c.cols) for c in cs}


def test_elementwise_and_rows_cases(caps):
    es = RC.elem_cases()
    big = 4 * RC.GRID1D_BLOCK * RC.GRID1D_CAP
    for op in ("gelu_fwd", "gelu_bwd", "dropout_f32", "dropout_bf16", "cast"):
        mine = [c for c in es if c.op == op]
        assert any(c.n > big for c in mine), f"{op}: no case with n > 4 * 256 * 4096 (the grid-stride loop)"
        assert {1, 5000} <= {c.n for c in mine}, op
        if op != "cast":
            assert {0.1, 0.25} <= {c.p for c in mine}, op
    rs = RC.rows_cases()
    for op in ("gather", "scatter"):
        assert {64, 1536} <= {c.cols for c in rs if c.op == op}
    assert any(c.op == "gather" and c.repeated for c in rs) and all(c.R == 700 for c in rs)
    assert any(c.cols > 128 * 8 for c in rs if c.op == "gather"), "gather: the column loop never comes round"


# ------------------------------------------------------------------------------------------------ argument errors
# Only calls that return BEFORE any HIP call are made here (read in rowops.hip: the check sits above the first
# hipLaunchKernelGGL / FBL_CHECK_LAUNCH of its entry point); pointers are never dereferenced on that path, so NULL will do.
def _ln_fwd(h, N, H):
    return h.fbl_ln_fwd(None, 0, 0.0, 0, None, None, None, None, None, None, None, None, None, 1e-7, None, None, None, None, None,
                        N, H, None)


def _ln_mat(h, N, H):
    return h.fbl_ln_materialize(None, None, None, None, None, None, 1, None, None, N, H, None)


def _ln_bwd(h, N, H, ld=0):
    return h.fbl_ln_bwd(None, None, None, None, None, 0.0, 0, None, None, None, None, None, None, None, None, N, H, ld, None)


@pytest.mark.parametrize("H", [0 + 63, 100, 1536 + 32, 2048 + 64, 4096])
def test_ln_rejects_h_not_multiple_of_64_or_over_2048(L, H):
    h = L.load()
    for N in (0, 5):  # the H check comes first: also for an empty call
        assert _ln_fwd(h, N, H) == ERR_SHAPE
        assert _ln_mat(h, N, H) == ERR_SHAPE
        assert _ln_bwd(h, N, H) == ERR_SHAPE


@pytest.mark.parametrize("H", [192, 320, 640, 1280, 1984])
def test_ln_rejects_h_without_an_instantiation(L, H):
    """H % 64 == 0 and H <= 2048 but H/64 is none of 1 2 4 8 12 16 24 32: the dispatch's default returns FBL_ERR_SHAPE without
    launching (a silent no-op would leave the outputs unwritten)"""
    h = L.load()
    assert _ln_fwd(h, 5, H) == ERR_SHAPE
    assert _ln_mat(h, 5, H) == ERR_SHAPE
    assert _ln_bwd(h, 5, H) == ERR_SHAPE
    # N <= 0 returns 0 after the H % 64 / H > 2048 check and before the dispatch: an empty call is not an error
    assert _ln_fwd(h, 0, H) == 0 and _ln_mat(h, 0, H) == 0 and _ln_bwd(h, 0, H) == 0


def test_ln_fwd_rejects_incomplete_r_norm(L):
    h = L.load()
    one = C.c_float(0.0)
    p = C.addressof(one)  # r_t given, its statistics / gamma / beta missing (never dereferenced)
    assert h.fbl_ln_fwd(None, 0, 0.0, 0, None, None, p, None, None, None, None, None, None, 1e-7, None, None, None, None, None,
                        5, 128, None) == ERR_ARG


@pytest.mark.parametrize("ld", [64, 1535, 1540, 1537])
def test_ln_bwd_rejects_a_bad_ld_dy_bf16(L, ld):
    """ld_dy_bf16 < H, or not a multiple of 8 (0 means H)"""
    assert _ln_bwd(L.load(), 5, 1536, ld) == ERR_ALIGN


def test_ce_bwd_rows_rejects_vp_below_v(L):
    h = L.load()
    assert h.fbl_ce_bwd_rows(None, 1024, None, None, 3, 1003, 1000, None, None, 1.0, None, None, None) == ERR_ARG
    assert h.fbl_ce_bwd_rows(None, 1024, None, None, 0, 1003, 1000, None, None, 1.0, None, None, None) == 0  # (R <= 0 first)


@pytest.mark.parametrize("cols,ld", [(60, 64), (64, 60), (1, 8)])
def test_gather_rows_rejects_unaligned(L, cols, ld):
    assert L.load().fbl_gather_rows_bf16(None, ld, None, 3, cols, None, None) == ERR_ALIGN


def test_sumsq_rejects_missing_buffers(L):
    assert L.load().fbl_sumsq(None, 5, None, None, None) == ERR_ARG


# Not testable without a GPU, because the launcher has nothing to reject (the kernels take any value): fbl_colsum,
# fbl_scatter_rows_f32, fbl_ce_fwd, fbl_adam_flat, fbl_cast_f32_to_bf16, fbl_dropout_* and fbl_dropout_gelu_* validate nothing
# beyond n <= 0 -> 0; a valid H in fbl_ln_* goes straight to a launch.
@pytest.mark.parametrize("call", [
    lambda h: h.fbl_colsum(None, 0, 8, 0, 8, None, None, None),
    lambda h: h.fbl_scatter_rows_f32(None, None, 0, 8, None, 8, None),
    lambda h: h.fbl_ce_fwd(None, 8, None, 0, 8, None, None, None),
    lambda h: h.fbl_adam_flat(None, None, None, None, 0, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, None, 0.0, 1.0, None),
    lambda h: h.fbl_cast_f32_to_bf16(None, None, 0, None),
    lambda h: h.fbl_dropout_f32(None, 0.1, 0, None, None, None, 0, None),
    lambda h: h.fbl_dropout_bf16(None, 0.0, 0, None, 100, None),
    lambda h: h.fbl_dropout_gelu_fwd(None, 0.1, 0, None, None, 0, None),
    lambda h: h.fbl_dropout_gelu_bwd(None, None, 0.1, 0, None, None, None, 0, None),
])
def test_empty_calls_return_zero_without_a_launch(L, call):
    assert call(L.load()) == 0
