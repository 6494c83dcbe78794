"""CPU: include/fbl_mha.h, lib.MHA_SIGNATURES and the built library agree on the four attention entry points of the BERT
variant, and the packed-row ones validate their arguments on the host before any launch (no GPU needed)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fbl_mha_fwd", "fbl_mha_bwd", "fbl_mha_fwd_rows", "fbl_mha_bwd_rows"}


def declared_functions():
    """the parser of tests/test_abi.py, pointed at include/fbl_mha.h"""
    src = open(os.path.join(ROOT, "include", "fbl_mha.h")).read()
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


def test_header_and_binding_agree_on_the_four_attention_entry_points():
    from frozenbilm_amd import lib

    decl = declared_functions()
    assert set(decl) == NAMES == set(lib.MHA_SIGNATURES), set(decl) ^ set(lib.MHA_SIGNATURES)
    for name, (ret, nargs) in decl.items():
        res, argtypes = lib.MHA_SIGNATURES[name]
        assert len(argtypes) == nargs, name
        assert ret == "int" and res is ctypes.c_int, name
    # the packed-row entry points: the padded ones plus row0 (forward) / plus O, ldo and row0 (backward)
    assert len(lib.MHA_SIGNATURES["fbl_mha_fwd_rows"][1]) == len(lib.MHA_SIGNATURES["fbl_mha_fwd"][1]) + 1 == 21
    assert len(lib.MHA_SIGNATURES["fbl_mha_bwd_rows"][1]) == len(lib.MHA_SIGNATURES["fbl_mha_bwd"][1]) + 3 == 30
    assert not NAMES & set(lib.SIGNATURES)  # include/fbl.h keeps its own table


def test_library_exports_the_four_attention_entry_points(libpath):
    h = ctypes.CDLL(libpath)
    for name in NAMES:
        assert hasattr(h, name), name
    from frozenbilm_amd import lib

    assert lib.load(libpath).fbl_abi_version() == lib.ABI_VERSION == 9  # adding functions changes no argument list


def test_packed_row_attention_rejects_bad_arguments_on_the_host(libpath):
    """row0 == NULL, klen == NULL, S = 513, a misaligned stride and p_drop = 1 are refused before any launch: the pointers are
    never dereferenced (no GPU needed)."""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)
    p, H = 0x1000, 768

    def fwd(row0=p, klen=p, S=64, ldq=3 * H, p_drop=0.0):
        return h.fbl_mha_fwd_rows(p, ldq, p, 3 * H, p, 3 * H, p, klen, None, row0, 0.125, p_drop, 0, None, p, H, p, 2, S, 12, None)

    def bwd(row0=p, klen=p, S=64, ldq=3 * H, p_drop=0.0, O=p):
        return h.fbl_mha_bwd_rows(p, ldq, p, 3 * H, p, 3 * H, p, H, O, H, p, klen, None, row0, p, p, 0.125, p_drop, 0, None,
                                  p, 3 * H, p, 3 * H, p, 3 * H, 2, S, 12, None)

    for call in (fwd, bwd):
        assert call(row0=None) < 0
        assert call(klen=None) < 0
        assert call(S=513) < 0 and call(S=0) < 0
        assert call(ldq=3 * H + 4) < 0
        assert call(p_drop=1.0) < 0 and call(p_drop=-0.5) < 0
    assert bwd(O=None) < 0
    # the codes are the padded entry points' (include/fbl.h FBL_ERR_*): shape -1, alignment -2
    assert fwd(S=513) == bwd(S=513) == -1
    assert fwd(ldq=3 * H + 4) == bwd(ldq=3 * H + 4) == -2
