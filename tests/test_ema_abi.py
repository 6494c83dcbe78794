"""CPU: include/fbl_ema.h, lib.EMA_SIGNATURES and the built library agree on fbl_adam_flat_groups_ema and fbl_swap_f32; the names
occur in no other signature table; the ABI stays at 9 and include/fbl.h keeps its 47 declarations; the argument rules return
their codes before any launch (the pointers are never dereferenced: no GPU needed).

Seen on the parent commit: test_header_and_binding_agree fails with FileNotFoundError (no include/fbl_ema.h),
test_library_exports_them_at_abi_9 with AssertionError at its `hasattr` line (the library exports neither name) and
test_bad_arguments_on_the_host with AttributeError (libfbl.so: undefined symbol: fbl_adam_flat_groups_ema)."""
import ctypes
import os

import pytest

from tests.test_groups_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fbl_adam_flat_groups_ema", "fbl_swap_f32"}
SHAPE, ALIGN, ARG = -1, -2, -3  # include/fbl.h FBL_ERR_*


@pytest.fixture(scope="module")
def libpath():
    from frozenbilm_amd.build import build_lib

    return build_lib(verbose=False)


def test_header_and_binding_agree():
    from frozenbilm_amd import lib

    decl = declared_functions("fbl_ema.h")
    assert set(decl) == NAMES == set(lib.EMA_SIGNATURES), set(decl) ^ set(lib.EMA_SIGNATURES)
    assert decl["fbl_adam_flat_groups_ema"] == ("int", 15) and decl["fbl_swap_f32"] == ("int", 4)
    vp, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert lib.EMA_SIGNATURES["fbl_adam_flat_groups_ema"] == (i, [vp, vp, vp, vp, vp, l, vp, i, vp, i, vp, f, f, f, vp])
    assert lib.EMA_SIGNATURES["fbl_swap_f32"] == (i, [vp, vp, l, vp])
    # the groups entry point's list with `ema` behind v and `ema_w` in front of the stream
    g = lib.GROUP_SIGNATURES["fbl_adam_flat_groups"][1]
    assert lib.EMA_SIGNATURES["fbl_adam_flat_groups_ema"][1] == g[:4] + [vp] + g[4:-1] + [f] + g[-1:]
    others = (lib.SIGNATURES, lib.MHA_SIGNATURES, lib.QROWS_SIGNATURES, lib.LIVE_SIGNATURES, lib.PREDICT_SIGNATURES,
              lib.GROUP_SIGNATURES, lib.LORA_SIGNATURES)
    assert not any(NAMES & set(t) for t in others)
    assert len(declared_functions("fbl.h")) == len(lib.SIGNATURES) == 47  # include/fbl.h keeps its declarations


def test_library_exports_them_at_abi_9(libpath):
    from frozenbilm_amd import build, lib

    h = ctypes.CDLL(libpath)
    for name in NAMES:
        assert hasattr(h, name), name
    assert lib.load(libpath).fbl_abi_version() == lib.ABI_VERSION == 9
    assert build._deps_mtime() >= os.path.getmtime(os.path.join(ROOT, "include", "fbl_ema.h"))


def test_bad_arguments_on_the_host(libpath):
    """NULL pointers (ema among them), n_groups outside 1 .. 64, ema_w outside (0, 1], a == b: FBL_ERR_ARG; n % 8 and a pointer
    off 16 bytes: FBL_ERR_ALIGN; n <= 0: 0 -- all before any launch"""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)
    a = 0x1000
    hyper = L.adam_hyper([(1e-3, 0.9, 0.95, 1e-8, 0.01, False)] * 3)

    def call(p=a, g=a, m=a, v=a, ema=a, n=64, segs=a, ng=3, hy=hyper, step=1, ss=None, max_norm=0.0, scale=1.0, w=0.1):
        return h.fbl_adam_flat_groups_ema(p, g, m, v, ema, n, segs, ng, hy, step, ss, max_norm, scale, w, None)

    assert call(n=0) == 0 and call(n=-8) == 0 and call(n=0, w=1.0) == 0
    for name in ("p", "g", "m", "v", "ema", "segs", "hy"):
        assert call(**{name: None}) == ARG, name
        assert call(**{name: None}, n=0) == ARG, name  # (validation comes first)
    assert call(ng=0) == ARG and call(ng=-1) == ARG and call(ng=65) == ARG
    for w in (0.0, -0.0, -0.1, 1.0 + 2.0 ** -23, 2.0, float("nan"), float("inf"), -float("inf")):
        assert call(w=w) == ARG and call(w=w, n=0) == ARG, w
    assert call(n=60) == ALIGN and call(n=4) == ALIGN
    for name in ("p", "g", "m", "v", "ema"):
        assert call(**{name: a + 4}) == ALIGN and call(**{name: a + 8}) == ALIGN, name
    assert call(ema=None, n=60) == ARG and call(w=0.0, n=60) == ARG  # argument rules before alignment

    def swap(x=a, y=a + 0x1000, n=64):
        return h.fbl_swap_f32(x, y, n, None)

    assert swap(n=0) == 0 and swap(n=-8) == 0
    assert swap(x=None) == ARG and swap(y=None) == ARG and swap(y=a) == ARG and swap(y=a, n=0) == ARG
    assert swap(n=60) == ALIGN and swap(n=4) == ALIGN
    assert swap(x=a + 4) == ALIGN and swap(y=a + 0x1008) == ALIGN
    assert swap(x=None, n=60) == ARG
