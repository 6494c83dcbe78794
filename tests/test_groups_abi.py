"""CPU: include/fbl_groups.h, lib.GROUP_SIGNATURES and the built library agree on fbl_adam_flat_groups; the ABI stays at 9 and
include/fbl.h keeps its 47 declarations; the argument rules return their codes before any launch (the pointers are never
dereferenced: no GPU needed); lib.group_table refuses a malformed segment list.

Seen on the parent commit: test_header_and_binding_agree fails with FileNotFoundError (no include/fbl_groups.h) and
test_group_table with AttributeError (module 'frozenbilm_amd.lib' has no attribute 'group_table'); the two tests on the built
library were not run there -- its library exports no fbl_adam_flat_groups and its `lib` has no adam_hyper, so the first stops at
its `hasattr` assertion and the second at AttributeError."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fbl_adam_flat_groups"}
SHAPE, ALIGN, ARG = -1, -2, -3  # include/fbl.h FBL_ERR_*


def declared_functions(header):
    """the parser of tests/test_abi.py, pointed at another header"""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|int64_t)\s+(fbl_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(3).strip()
        n = 0 if args in ("", "void") else args.count(",") + 1
        out[m.group(2)] = (m.group(1), n)
    return out


@pytest.fixture(scope="module")
def libpath():
    from frozenbilm_amd.build import build_lib

    return build_lib(verbose=False)


def test_header_and_binding_agree():
    from frozenbilm_amd import lib

    decl = declared_functions("fbl_groups.h")
    assert set(decl) == NAMES == set(lib.GROUP_SIGNATURES), set(decl) ^ set(lib.GROUP_SIGNATURES)
    assert decl["fbl_adam_flat_groups"] == ("int", 13)
    vp, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert lib.GROUP_SIGNATURES["fbl_adam_flat_groups"] == (i, [vp, vp, vp, vp, l, vp, i, vp, i, vp, f, f, vp])
    assert not NAMES & (set(lib.SIGNATURES) | set(lib.MHA_SIGNATURES) | set(lib.QROWS_SIGNATURES) | set(lib.LIVE_SIGNATURES)
                        | set(lib.PREDICT_SIGNATURES))
    assert len(declared_functions("fbl.h")) == len(lib.SIGNATURES) == 47  # include/fbl.h keeps its declarations
    src = open(os.path.join(ROOT, "include", "fbl_groups.h")).read()
    assert int(re.search(r"#define FBL_ADAM_MAX_GROUPS (\d+)", src).group(1)) == lib.ADAM_MAX_GROUPS == 64
    assert int(re.search(r"#define FBL_ADAM_GROUP_FLOATS (\d+)", src).group(1)) == lib.ADAM_GROUP_FLOATS == 6


def test_library_exports_it_at_abi_9(libpath):
    from frozenbilm_amd import build, lib

    h = ctypes.CDLL(libpath)
    for name in NAMES:
        assert hasattr(h, name), name
    assert lib.load(libpath).fbl_abi_version() == lib.ABI_VERSION == 9
    assert build._deps_mtime() >= os.path.getmtime(os.path.join(ROOT, "include", "fbl_groups.h"))


def test_bad_arguments_on_the_host(libpath):
    """NULL pointers, n_groups outside 1 .. 64 and a NULL hyper array: FBL_ERR_ARG; n % 8 and a pointer off 16 bytes:
    FBL_ERR_ALIGN; n <= 0: 0 -- all before any launch"""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)
    a = 0x1000
    hyper = L.adam_hyper([(1e-3, 0.9, 0.95, 1e-8, 0.01, False)] * 3)

    def call(p=a, g=a, m=a, v=a, n=64, segs=a, ng=3, hy=hyper, step=1, ss=None, max_norm=0.0, scale=1.0):
        return h.fbl_adam_flat_groups(p, g, m, v, n, segs, ng, hy, step, ss, max_norm, scale, None)

    assert call(n=0) == 0 and call(n=-8) == 0
    for name in ("p", "g", "m", "v", "segs", "hy"):
        assert call(**{name: None}) == ARG, name
        assert call(**{name: None}, n=0) == ARG, name  # (validation comes first)
    assert call(ng=0) == ARG and call(ng=-1) == ARG and call(ng=65) == ARG
    assert call(n=60) == ALIGN and call(n=4) == ALIGN
    for name in ("p", "g", "m", "v"):
        assert call(**{name: a + 4}) == ALIGN and call(**{name: a + 8}) == ALIGN, name
    assert call(p=None, n=60) == ARG  # argument rules before alignment


def test_group_table():
    from frozenbilm_amd import lib as L

    tab = L.group_table([(0, 8, 2), (16, 32, 0), (32, 40, 1)], 48, "cpu")
    assert tab.dtype is __import__("torch").int64
    assert tab.tolist() == [3, 32, 0, 0, 2, 16, 8, 0, 32, 24, 1]
    assert L.group_table([], 48, "cpu").tolist() == [0, 0]
    for bad in ([(0, 12, 0)], [(8, 16, 0), (0, 8, 0)], [(0, 16, 0), (8, 24, 1)], [(0, 8, 0), (8, 8, 0)], [(0, 56, 0)],
                [(0, 8, -1)], [(0, 8, 64)], [(4, 12, 0)]):
        with pytest.raises(ValueError):
            L.group_table(bad, 48, "cpu")
    with pytest.raises(ValueError):
        L.group_table([(0, 8, 2)], 48, "cpu", n_groups=2)  # a group id the call would not know
    with pytest.raises(ValueError):
        L.group_table([(8 * i, 8 * i + 8, 0) for i in range(0, 2 * 1025, 2)], 8 * 2 * 1025, "cpu")  # more than 1024 segments
    with pytest.raises(ValueError):
        L.adam_hyper([(1e-3, 0.9, 0.95, 1e-8, 0.0, False)] * 65)
    assert list(L.adam_hyper([(0.5, 0.25, 0.125, 2.0, 4.0, True)])) == [0.5, 0.25, 0.125, 2.0, 4.0, 1.0]
