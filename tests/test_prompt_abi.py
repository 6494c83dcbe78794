"""CPU: include/fbl_prompt.h, lib.PROMPT_SIGNATURES and the built library agree on the two prompt-tuning entry points; the ABI
stays at 9 and include/fbl.h keeps its 47 declarations; bad arguments are refused on the host, before any launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fbl_embed_assemble", "fbl_prompt_grad"}


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

    decl = declared_functions("fbl_prompt.h")
    assert set(decl) == NAMES == set(lib.PROMPT_SIGNATURES), set(decl) ^ set(lib.PROMPT_SIGNATURES)
    vp, i = ctypes.c_void_p, ctypes.c_int
    res, argtypes = lib.PROMPT_SIGNATURES["fbl_embed_assemble"]
    assert decl["fbl_embed_assemble"] == ("int", 11) and res is i
    assert argtypes == [vp, vp, vp, vp, i, i, i, i, i, vp, vp]  # ids, E, vproj, prompt, B, T, P, L, H, out_t, stream
    res, argtypes = lib.PROMPT_SIGNATURES["fbl_prompt_grad"]
    assert decl["fbl_prompt_grad"] == ("int", 9) and res is i
    assert argtypes == [vp, vp, i, i, i, i, i, vp, vp]  # dt, row0, B, S, T, P, H, g, stream
    others = (set(lib.SIGNATURES) | set(lib.MHA_SIGNATURES) | set(lib.QROWS_SIGNATURES) | set(lib.LIVE_SIGNATURES)
              | set(lib.PREDICT_SIGNATURES) | set(lib.GROUP_SIGNATURES) | set(lib.LORA_SIGNATURES) | set(lib.EMA_SIGNATURES))
    assert not NAMES & others
    assert len(declared_functions("fbl.h")) == len(lib.SIGNATURES) == 47  # include/fbl.h keeps its declarations
    src = open(os.path.join(ROOT, "include", "fbl_prompt.h")).read()
    from frozenbilm_amd.model import deberta

    assert int(re.search(r"#define FBL_PROMPT_MAX (\d+)", src).group(1)) == lib.PROMPT_MAX == deberta.PROMPT_MAX == 128


def test_library_exports_them_at_abi_9(libpath):
    from frozenbilm_amd import build, lib

    h = ctypes.CDLL(libpath)
    for name in NAMES:
        assert hasattr(h, name), name
    assert lib.load(libpath).fbl_abi_version() == lib.ABI_VERSION == 9
    assert build._deps_mtime() >= os.path.getmtime(os.path.join(ROOT, "include", "fbl_prompt.h"))
    assert os.path.join(build.CSRC, "prompt.hip") in build.sources()


ARG, ALIGN, SHAPE = -3, -2, -1
PTR = 0x10000


def test_embed_assemble_refusals(libpath):
    """H off the 16-byte piece, P outside 1..128, a NULL prompt, a misaligned pointer and T > 0 without vproj are refused before
    any launch, an empty grid returns 0 and launches nothing: the pointers are never dereferenced (no GPU needed)"""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)

    def call(**kw):
        a = dict(ids=PTR, E=PTR, vproj=PTR, prompt=PTR, B=0, T=2, P=5, L=7, H=64, out=PTR)
        a.update(kw)
        return h.fbl_embed_assemble(a["ids"], a["E"], a["vproj"], a["prompt"], a["B"], a["T"], a["P"], a["L"], a["H"], a["out"], None)

    assert call() == 0 and call(ids=None, E=None) == 0 and call(T=0, vproj=None) == 0  # B = 0: nothing to launch
    assert call(H=66) == call(H=0) == call(H=-4) == SHAPE
    assert call(H=66, P=0) == SHAPE  # (checked in the documented order)
    assert call(P=0) == call(P=129) == call(P=-1) == ARG
    assert call(prompt=None) == call(out=None) == call(E=None) == ARG
    assert call(B=-1) == call(T=-1, vproj=None) == call(L=-1) == ARG
    assert call(prompt=PTR + 4) == call(out=PTR + 8) == call(E=PTR + 4) == call(vproj=PTR + 12) == call(ids=PTR + 4) == ALIGN
    assert call(vproj=None) == ARG and call(vproj=None, B=3) == ARG
    assert call(prompt=PTR + 4, vproj=None) == ALIGN  # (alignment is checked before the missing vproj)
    assert call(B=1 << 20, L=1 << 20) == SHAPE  # more than 2^31 - 1 rows


def test_prompt_grad_refusals(libpath):
    from frozenbilm_amd import lib as L

    h = L.load(libpath)

    def call(**kw):
        a = dict(dt=PTR, row0=None, B=0, S=14, T=2, P=5, H=64, g=PTR)
        a.update(kw)
        return h.fbl_prompt_grad(a["dt"], a["row0"], a["B"], a["S"], a["T"], a["P"], a["H"], a["g"], None)

    assert call() == 0 and call(row0=PTR) == 0  # B = 0: nothing to launch
    assert call(H=66) == call(H=0) == SHAPE
    assert call(S=6) == SHAPE and call(S=6, row0=PTR) == 0  # (S is the padded grid's; packed rows carry their own offsets)
    assert call(P=0) == call(P=129) == ARG
    assert call(dt=None) == call(g=None) == call(B=-1) == call(T=-1) == ARG
    assert call(dt=PTR + 4) == call(g=PTR + 8) == call(row0=PTR + 2) == ALIGN
