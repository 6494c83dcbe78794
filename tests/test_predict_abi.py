"""CPU: include/fbl_predict.h, lib.PREDICT_SIGNATURES and the built library agree on the row-prediction entry points; the ABI
stays at 9 and include/fbl.h keeps its 47 declarations; bad arguments are refused on the host."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fbl_row_predict", "fbl_row_predict_ws_bytes"}


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

    decl = declared_functions("fbl_predict.h")
    assert set(decl) == NAMES == set(lib.PREDICT_SIGNATURES), set(decl) ^ set(lib.PREDICT_SIGNATURES)
    for name, (ret, nargs) in decl.items():
        res, argtypes = lib.PREDICT_SIGNATURES[name]
        assert len(argtypes) == nargs, name
        assert {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[ret] is res, name
    assert decl["fbl_row_predict"] == ("int", 14) and decl["fbl_row_predict_ws_bytes"] == ("int64_t", 3)
    assert not NAMES & (set(lib.SIGNATURES) | set(lib.MHA_SIGNATURES) | set(lib.QROWS_SIGNATURES) | set(lib.LIVE_SIGNATURES))
    assert len(declared_functions("fbl.h")) == len(lib.SIGNATURES) == 47  # include/fbl.h keeps its declarations
    src = open(os.path.join(ROOT, "include", "fbl_predict.h")).read()
    assert int(re.search(r"#define FBL_PREDICT_MAX_K (\d+)", src).group(1)) == lib.PREDICT_MAX_K == 16


def test_library_exports_them_at_abi_9(libpath):
    from frozenbilm_amd import build, lib

    h = ctypes.CDLL(libpath)
    for name in NAMES:
        assert hasattr(h, name), name
    assert lib.load(libpath).fbl_abi_version() == lib.ABI_VERSION == 9
    assert build._deps_mtime() >= os.path.getmtime(os.path.join(ROOT, "include", "fbl_predict.h"))
    assert os.path.join(build.CSRC, "predict.hip") in build.sources()


def test_workspace_size_and_bad_arguments_on_the_host(libpath):
    """the workspace formula; NULL buffers, k outside 1..16, a bad shape, a misaligned pointer and a short workspace are refused
    before any launch; R = 0 returns 0 and launches nothing: the pointers are never dereferenced (no GPU needed)"""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)
    p = 0x1000
    per_chunk = lambda k: 8 * k + 12  # noqa: E731  (k keys, (max, sum), one count)
    assert h.fbl_row_predict_ws_bytes(3, 128100, 5) == 3 * 16 * per_chunk(5)
    assert h.fbl_row_predict_ws_bytes(7, 8192, 16) == 7 * 1 * per_chunk(16)
    assert h.fbl_row_predict_ws_bytes(7, 8193, 1) == 7 * 2 * per_chunk(1)
    assert h.fbl_row_predict_ws_bytes(0, 100, 5) == 0
    assert h.fbl_row_predict_ws_bytes(3, 0, 5) == -1 and h.fbl_row_predict_ws_bytes(3, 100, 0) == -3
    assert h.fbl_row_predict_ws_bytes(3, 100, 17) == -3

    def call(x=p, ldv=128, R=4, V=100, k=5, lab=None, lse=None, ids=p, lp=p, rank=None, nll=None, ws=p, nb=1 << 20):
        return h.fbl_row_predict(x, ldv, R, V, k, lab, lse, ids, lp, rank, nll, ws, nb, None)

    assert call(R=0) == 0 and call(R=0, x=None, ids=None, lp=None, ws=None) == 0
    assert call(x=None) == call(ids=None) == call(lp=None) == call(ws=None) == -3
    assert call(k=0) == call(k=17) == -3
    assert call(lab=p) == call(lab=p, rank=p) == call(lab=p, nll=p) == -3        # labels need both outputs
    assert call(rank=p) == call(nll=p) == call(rank=p, nll=p) == -3              # ... and the outputs need labels
    assert call(V=0) == call(V=129) == call(R=-1) == -1
    assert call(ldv=130, V=100) == call(x=p + 4) == call(ws=p + 4) == -2
    assert call(nb=4 * per_chunk(5) - 1) == -3
