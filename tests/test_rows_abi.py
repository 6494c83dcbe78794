"""CPU: include/fbl_rows.h (the compact row layout of the backward pass) -- the binding's argument types come from the header, the
library exports the three entry points, and each of them validates its arguments before any HIP call (pointers are never
dereferenced on these paths: no GPU needed)."""
import ctypes

import pytest

SHAPE, ALIGN, ARG = -1, -2, -3  # include/fbl.h FBL_ERR_*


@pytest.fixture(scope="module")
def h():
    from frozenbilm_amd import lib
    from frozenbilm_amd.build import build_lib

    return lib.load(build_lib(verbose=False))


def test_signatures_come_from_the_header():
    from frozenbilm_amd import lib

    vp, i, l, f, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64
    assert set(lib.ROWS_SIGNATURES) == {"fbl_ln_bwd_rows", "fbl_gather_rows_multi", "fbl_scatter_rows_zero_bf16"}
    assert lib.ROWS_SIGNATURES["fbl_ln_bwd_rows"] == (i, [vp, vp, vp, vp, vp, vp, f, u, vp, vp, vp, l, vp, vp, vp, vp, vp, i, i, vp])
    assert lib.ROWS_SIGNATURES["fbl_gather_rows_multi"] == (i, [i, vp, vp, vp, vp, vp, vp, i, vp])
    assert lib.ROWS_SIGNATURES["fbl_scatter_rows_zero_bf16"] == (i, [vp, l, vp, i, i, vp, l, vp])
    assert not set(lib.ROWS_SIGNATURES) & set(lib.SIGNATURES)
    assert lib.GATHER_MAX_TENSORS == 8


def test_ln_bwd_rows_rejects_bad_arguments(h):
    p = 0x1000

    def call(H=1536, N=5, ld=0, inv=p, pad=p, dout=p, ws=p):
        return h.fbl_ln_bwd_rows(dout, inv, None, p, p, p, 0.0, 0, None, None, None, ld, pad, None, None, None, ws, N, H, None)

    for H in (63, 100, 2048 + 64):
        assert call(H=H) == SHAPE and call(H=H, N=0) == SHAPE
    assert call(inv=None) == ARG and call(pad=None) == ARG and call(dout=None) == ARG and call(ws=None) == ARG
    assert call(N=0) == 0  # an empty call: nothing launched
    assert call(ld=1540) == ALIGN and call(ld=1024) == ALIGN  # not a multiple of 8; smaller than H


def test_gather_rows_multi_rejects_bad_arguments(h):
    p = 0x1000
    tab = lambda *v: (ctypes.c_void_p * len(v))(*v)
    arr = lambda *v: (ctypes.c_int64 * len(v))(*v)

    def call(n=2, src=tab(p, p), dst=tab(p, p), rb=arr(384, 8), sl=arr(384, 8), dl=arr(384, 8), sel=p, Np=0):
        return h.fbl_gather_rows_multi(n, src, dst, rb, sl, dl, sel, Np, None)

    assert call() == 0  # valid tables, no row: nothing launched
    assert call(n=0) == ARG and call(n=9) == ARG
    assert call(src=None) == ARG and call(sel=None) == ARG and call(src=tab(p, None)) == ARG
    assert call(rb=arr(384, 0)) == ARG                       # an empty row
    assert call(sl=arr(256, 8)) == ARG and call(dl=arr(384, 4)) == ARG  # a stride smaller than its row
    assert call(rb=arr(384, 6), sl=arr(384, 6), dl=arr(384, 6)) == ALIGN  # 4-byte pieces at least
    assert call(src=tab(p + 2, p)) == ALIGN


def test_scatter_rows_zero_rejects_bad_arguments(h):
    p = 0x1000

    def call(src=p, lds=192, inv=p, N=5, cols=192, dst=p, ldd=192):
        return h.fbl_scatter_rows_zero_bf16(src, lds, inv, N, cols, dst, ldd, None)

    assert call(N=0) == 0 and call(cols=0) == 0
    assert call(src=None) == ARG and call(inv=None) == ARG and call(dst=None) == ARG
    assert call(lds=128) == ARG and call(ldd=64) == ARG
    assert call(cols=100, lds=104, ldd=104) == ALIGN and call(lds=196) == ALIGN and call(dst=p + 8) == ALIGN
