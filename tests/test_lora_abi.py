"""CPU: include/fbl_lora.h, lib.LORA_SIGNATURES and the built library agree on the LoRA compose entry point; the ABI stays at 9
and include/fbl.h keeps its 47 declarations; bad arguments are refused on the host, before any launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fbl_lora_compose"}


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

    decl = declared_functions("fbl_lora.h")
    assert set(decl) == NAMES == set(lib.LORA_SIGNATURES), set(decl) ^ set(lib.LORA_SIGNATURES)
    res, argtypes = lib.LORA_SIGNATURES["fbl_lora_compose"]
    assert decl["fbl_lora_compose"] == ("int", 4) and res is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    others = (set(lib.SIGNATURES) | set(lib.MHA_SIGNATURES) | set(lib.QROWS_SIGNATURES) | set(lib.LIVE_SIGNATURES)
              | set(lib.PREDICT_SIGNATURES) | set(lib.GROUP_SIGNATURES))
    assert not NAMES & others
    assert len(declared_functions("fbl.h")) == len(lib.SIGNATURES) == 47  # include/fbl.h keeps its declarations
    src = open(os.path.join(ROOT, "include", "fbl_lora.h")).read()
    assert int(re.search(r"#define FBL_LORA_MAX_RANK (\d+)", src).group(1)) == lib.LORA_MAX_RANK == 64
    assert int(re.search(r"#define FBL_LORA_SITE_WORDS (\d+)", src).group(1)) == lib.LORA_SITE_WORDS == 16


def test_library_exports_it_at_abi_9(libpath):
    from frozenbilm_amd import build, lib

    h = ctypes.CDLL(libpath)
    for name in NAMES:
        assert hasattr(h, name), name
    assert lib.load(libpath).fbl_abi_version() == lib.ABI_VERSION == 9
    assert build._deps_mtime() >= os.path.getmtime(os.path.join(ROOT, "include", "fbl_lora.h"))
    assert os.path.join(build.CSRC, "lora.hip") in build.sources()


def test_bad_arguments_are_refused_on_the_host(libpath):
    """NULL tables and pointers, a rank outside 1..64, shapes off the 64-tile, short or misaligned leading dimensions and
    misaligned pointers are refused before any launch; no site returns 0 and launches nothing: the pointers are never
    dereferenced (no GPU needed)"""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)
    p = 0x10000
    ARG, ALIGN, SHAPE = -3, -2, -1

    def call(n=1, dev=p, host=True, **kw):
        rec = dict(W=p, ldw=128, A=p, B=p, dst=p, ld_dst=128, dstT=p, ld_dstT=192, d32=0, ld32=0, O=192, I=128, r=8, s=0)
        rec.update(kw)
        words = [rec[k] for k in ("W", "ldw", "A", "B", "dst", "ld_dst", "dstT", "ld_dstT", "d32", "ld32", "O", "I", "r", "s")] + [0, 0]
        tab = (ctypes.c_int64 * (16 * max(n, 1)))(*(words * max(n, 1)))
        return h.fbl_lora_compose(tab if host else None, dev, n, None)

    assert call(n=0) == 0 and call(n=0, dev=None, host=False) == 0
    assert call(n=-1) == call(n=4097) == ARG
    assert call(dev=None) == call(host=False) == ARG
    assert call(W=0) == call(A=0) == call(B=0) == call(dst=0) == call(dstT=0) == ARG
    assert call(r=0) == call(r=65) == call(r=-1) == ARG
    assert call(O=100) == call(I=96) == call(O=0) == call(I=0) == SHAPE
    assert call(ldw=64) == call(ld_dst=64) == call(ld_dstT=128) == call(d32=p, ld32=64) == SHAPE
    assert call(ldw=130) == call(ld_dst=132) == call(ld_dstT=196) == call(d32=p, ld32=130) == ALIGN
    assert call(W=p + 4) == call(A=p + 8) == call(dst=p + 2) == call(dstT=p + 8) == call(d32=p + 4, ld32=128) == call(B=p + 2) == ALIGN
    assert call(n=3, r=65) == ARG  # (every site is checked)
