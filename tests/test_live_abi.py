"""CPU: include/fbl_live.h, lib.LIVE_SIGNATURES and the built library agree on the two live-set entry points (clip norm and Adam
over a live set of the flat buffer); include/fbl.h keeps its 47 declarations at ABI 9; bad arguments are refused on the host."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fbl_sumsq_live", "fbl_adam_flat_live"}


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

    decl = declared_functions("fbl_live.h")
    assert set(decl) == NAMES == set(lib.LIVE_SIGNATURES), set(decl) ^ set(lib.LIVE_SIGNATURES)
    assert len(decl) == 2
    for name, (ret, nargs) in decl.items():
        res, argtypes = lib.LIVE_SIGNATURES[name]
        assert len(argtypes) == nargs, name
        assert {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[ret] is res, name
    assert decl["fbl_sumsq_live"][1] == 6 and decl["fbl_adam_flat_live"][1] == 16  # fbl_sumsq / fbl_adam_flat + the table
    assert not NAMES & (set(lib.SIGNATURES) | set(lib.MHA_SIGNATURES) | set(lib.QROWS_SIGNATURES))
    assert len(declared_functions("fbl.h")) == len(lib.SIGNATURES) == 47  # include/fbl.h keeps its declarations


def test_library_exports_them_at_abi_9(libpath):
    from frozenbilm_amd import build, lib

    h = ctypes.CDLL(libpath)
    for name in NAMES:
        assert hasattr(h, name), name
    assert lib.load(libpath).fbl_abi_version() == lib.ABI_VERSION == 9
    hdr = os.path.join(ROOT, "include", "fbl_live.h")
    assert build._deps_mtime() >= os.path.getmtime(hdr)


def test_bad_arguments_are_refused_on_the_host(libpath):
    """NULL buffers / table / workspace, an n that is no multiple of 8 and a misaligned pointer are refused before any launch;
    n = 0 returns 0: the pointers are never dereferenced (no GPU needed)."""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)
    p = 0x1000

    def ss(x=p, n=64, tab=p, out=p, ws=p):
        return h.fbl_sumsq_live(x, n, tab, out, ws, None)

    def adam(pp=p, g=p, m=p, v=p, n=64, tab=p):
        return h.fbl_adam_flat_live(pp, g, m, v, n, tab, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, None, 0.0, 1.0, None)

    assert ss(n=0) == 0 and adam(n=0) == 0
    assert ss(x=None) == ss(tab=None) == ss(out=None) == ss(ws=None) == -3
    assert adam(pp=None) == adam(g=None) == adam(m=None) == adam(v=None) == adam(tab=None) == -3
    assert ss(n=60) == adam(n=60) == -2
    assert ss(x=p + 4) == adam(pp=p + 8) == adam(g=p + 4) == adam(m=p + 4) == adam(v=p + 12) == -2


def test_live_table_layout():
    from frozenbilm_amd import lib as L

    assert L.live_table([(0, 8), (16, 32)], 32, "cpu").tolist() == [2, 24, 0, 0, 16, 8]
    assert L.live_table([], 32, "cpu").tolist() == [0, 0]
    for bad in ([(0, 12)], [(8, 16), (0, 8)], [(0, 16), (8, 24)], [(0, 8), (8, 8)], [(0, 40)], [(4, 12)]):
        with pytest.raises(ValueError):
            L.live_table(bad, 32, "cpu")
    with pytest.raises(ValueError):
        L.live_table([(16 * i, 16 * i + 8) for i in range(L.LIVE_MAX_RANGES + 1)], 16 * (L.LIVE_MAX_RANGES + 1), "cpu")
