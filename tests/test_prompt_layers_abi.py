"""CPU: include/fbl_prompt_layers.h, lib.PROMPT_LAYERS_SIGNATURES and the built library agree on the two entry points of deep
prompt tuning; the ABI stays at 9, include/fbl.h keeps its 47 declarations and include/fbl_prompt.h its two; bad arguments are
refused on the host in the documented order, before any launch."""
import ctypes
import os

import pytest

from tests.test_prompt_abi import ALIGN, ARG, PTR, ROOT, SHAPE, declared_functions

NAMES = {"fbl_prompt_rows_write", "fbl_prompt_rows_grad"}


@pytest.fixture(scope="module")
def libpath():
    from frozenbilm_amd.build import build_lib

    return build_lib(verbose=False)


def test_header_and_binding_agree():
    from frozenbilm_amd import lib

    decl = declared_functions("fbl_prompt_layers.h")
    assert set(decl) == NAMES == set(lib.PROMPT_LAYERS_SIGNATURES), set(decl) ^ set(lib.PROMPT_LAYERS_SIGNATURES)
    vp, i = ctypes.c_void_p, ctypes.c_int
    res, argtypes = lib.PROMPT_LAYERS_SIGNATURES["fbl_prompt_rows_write"]
    assert decl["fbl_prompt_rows_write"] == ("int", 10) and res is i
    assert argtypes == [vp, vp, i, i, i, i, i, vp, vp, vp]  # prompt, row0, B, S, T, P, H, out_f32, out_bf16, stream
    res, argtypes = lib.PROMPT_LAYERS_SIGNATURES["fbl_prompt_rows_grad"]
    assert decl["fbl_prompt_rows_grad"] == ("int", 9) and res is i
    assert argtypes == [vp, vp, i, i, i, i, i, vp, vp]  # dx, row0, B, S, T, P, H, g, stream
    others = (set(lib.SIGNATURES) | set(lib.MHA_SIGNATURES) | set(lib.QROWS_SIGNATURES) | set(lib.LIVE_SIGNATURES)
              | set(lib.PREDICT_SIGNATURES) | set(lib.GROUP_SIGNATURES) | set(lib.LORA_SIGNATURES) | set(lib.EMA_SIGNATURES)
              | set(lib.PROMPT_SIGNATURES) | set(lib.ROWS_SIGNATURES))
    assert not NAMES & others


def test_the_older_tables_are_unchanged():
    from frozenbilm_amd import lib

    assert set(lib.PROMPT_SIGNATURES) == set(declared_functions("fbl_prompt.h")) == {"fbl_embed_assemble", "fbl_prompt_grad"}
    assert len(declared_functions("fbl.h")) == len(lib.SIGNATURES) == 47
    assert lib.ABI_VERSION == 9


def test_library_exports_them_at_abi_9(libpath):
    from frozenbilm_amd import build, lib

    h = ctypes.CDLL(libpath)
    for name in NAMES | set(lib.PROMPT_SIGNATURES):
        assert hasattr(h, name), name
    assert lib.load(libpath).fbl_abi_version() == lib.ABI_VERSION == 9
    assert build._deps_mtime() >= os.path.getmtime(os.path.join(ROOT, "include", "fbl_prompt_layers.h"))
    assert os.path.join(build.CSRC, "prompt_layers.hip") in build.sources()


def test_rows_write_refusals(libpath):
    """every refusal in the header's order; B = 0 returns 0 and launches nothing: the pointers are never dereferenced"""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)

    def call(**kw):
        a = dict(prompt=PTR, row0=None, B=0, S=14, T=2, P=5, H=64, f32=PTR, bf16=PTR)
        a.update(kw)
        return h.fbl_prompt_rows_write(a["prompt"], a["row0"], a["B"], a["S"], a["T"], a["P"], a["H"], a["f32"], a["bf16"], None)

    assert call() == 0 and call(row0=PTR) == 0 and call(f32=None) == 0 and call(bf16=None) == 0  # B = 0: nothing to launch
    assert call(H=66) == call(H=0) == call(H=-4) == SHAPE
    assert call(H=66, P=0) == SHAPE  # (the shape of H comes first)
    assert call(P=0) == call(P=129) == call(P=-1) == ARG
    assert call(prompt=None) == call(f32=None, bf16=None) == call(B=-1) == call(T=-1) == ARG
    assert call(P=0, S=1) == ARG and call(prompt=None, S=1) == ARG  # (arguments before the grid's shape)
    assert call(S=6) == SHAPE and call(S=6, row0=PTR) == 0  # (S is the padded grid's; packed rows carry their own offsets)
    assert call(B=1 << 30, P=128) == SHAPE  # more than 2^31 - 1 (b, p) pairs
    assert call(S=6, prompt=PTR + 4) == SHAPE  # (shape before alignment)
    assert call(prompt=PTR + 4) == call(f32=PTR + 8) == call(bf16=PTR + 4) == call(row0=PTR + 2) == ALIGN
    assert call(bf16=PTR + 8) == 0  # the bf16 rows are stored in 8-byte pieces


def test_rows_grad_refusals(libpath):
    from frozenbilm_amd import lib as L

    h = L.load(libpath)

    def call(**kw):
        a = dict(dx=PTR, row0=None, B=0, S=14, T=2, P=5, H=64, g=PTR)
        a.update(kw)
        return h.fbl_prompt_rows_grad(a["dx"], a["row0"], a["B"], a["S"], a["T"], a["P"], a["H"], a["g"], None)

    assert call() == 0 and call(row0=PTR) == 0  # B = 0: nothing to launch
    assert call(g=None) == 0  # a frozen prompt: the rows are cleared only
    assert call(H=66) == call(H=0) == SHAPE
    assert call(H=66, P=0) == SHAPE
    assert call(P=0) == call(P=129) == ARG
    assert call(dx=None) == call(B=-1) == call(T=-1) == ARG
    assert call(dx=None, S=6) == ARG  # (arguments before the grid's shape)
    assert call(S=6) == SHAPE and call(S=6, row0=PTR) == 0
    assert call(S=6, dx=PTR + 4) == SHAPE  # (shape before alignment)
    assert call(dx=PTR + 4) == call(g=PTR + 8) == call(row0=PTR + 2) == ALIGN
