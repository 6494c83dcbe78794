"""CPU: the C-ABI shared library builds, loads and exports exactly what include/fbl.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "fbl.h")).read()
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


def test_header_and_binding_agree_on_47_exports(libpath):
    """include/fbl.h and lib.SIGNATURES declare the same 47 entry points (46 + the plan query fbl_gemm_plan_launches) with the
    same argument counts and return types."""
    from frozenbilm_amd import lib

    decl = declared_functions()
    assert len(decl) == 47
    assert set(decl) == set(lib.SIGNATURES), set(decl) ^ set(lib.SIGNATURES)
    for name, (ret, nargs) in decl.items():
        res, argtypes = lib.SIGNATURES[name]
        assert len(argtypes) == nargs, name
        assert (res is ctypes.c_int64) == (ret == "int64_t"), name


def test_binding_argument_types_come_from_the_headers():
    """lib.*SIGNATURES are parsed from the C declarations: one hand-written type list per header against the derived one (the
    count-based parser above cannot tell a c_int from a c_int64), and a type outside the map is an error, not a guess."""
    from frozenbilm_amd import lib

    vp, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert lib.SIGNATURES["fbl_gemm_plan"] == (i, [i, i, i, i, i])
    assert lib.SIGNATURES["fbl_sumsq"] == (i, [vp, l, vp, vp, vp])
    assert lib.MHA_SIGNATURES["fbl_mha_fwd_rows"] == (
        i, [vp, l, vp, l, vp, l, vp, vp, vp, vp, f, f, ctypes.c_uint64, vp, vp, l, vp, i, i, i, vp])
    assert lib.QROWS_SIGNATURES["fbl_disent_attn_bwd_qrows_ws_bytes"] == (l, [i, i, i])
    assert lib.parse_signatures("int64_t fbl_a(const void* const* x, uint64_t s, float);") == {
        "fbl_a": (l, [vp, ctypes.c_uint64, f])}
    with pytest.raises(ValueError, match="fbl_bad"):
        lib.parse_signatures("int fbl_ok(int n);\nint fbl_bad(const void* p, double x);")
    with pytest.raises(ValueError, match="fbl_bad"):
        lib.parse_signatures("unsigned fbl_bad(int n);")
    for odd in ("int fbl_bad(int x[4]);", "int fbl_bad(void (*f)(void), int n);"):  # never dropped from the table in silence
        with pytest.raises(ValueError, match="fbl_bad"):
            lib.parse_signatures("int fbl_ok(int n);\n" + odd)


def test_library_exports_every_symbol(libpath):
    h = ctypes.CDLL(libpath)
    for name in declared_functions():
        assert hasattr(h, name), name
    from frozenbilm_amd import lib

    handle = lib.load(libpath)
    assert handle.fbl_abi_version() == lib.ABI_VERSION == 9  # (lib.load refuses any other library: argument lists differ)
    assert handle.fbl_ln_bwd_ws_floats(1536) == 768 * 3 * 1536
    assert handle.fbl_colsum_ws_floats(100) == 512 * 100


def test_product_library_reads_no_environment(libpath):
    """The experiment switches (FBL_GEMM8_VAR, FBL_ATTN_*) exist only in FBL_DEBUG_BUILD=1 builds: the product library
    does not even import getenv, and owns no stream (no hipStreamCreate*: helper streams are caller-provided)."""
    import subprocess

    syms = subprocess.run(["nm", "-D", "--undefined-only", libpath], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in syms
    assert "hipStreamCreate" not in syms
    # ... and every entry point is kernel launches (+ event fork / join onto the caller's aux stream) only: no memset / memcpy /
    # allocation calls.  A captured training step then consists of kernel nodes, ordered like eager launches -- the zero fills of the
    # accumulation targets were hipMemsetAsync for a while (memset nodes in the graphs) and replayed steps produced non-finite
    # gradients about once in 500 replays.
    for forbidden in ("hipMemset", "hipMemcpy", "hipMalloc", "hipFree", "hipHostMalloc", "hipDeviceSynchronize", "hipStreamSynchronize"):
        assert forbidden not in syms, forbidden


def test_missing_library_fails_loudly(tmp_path):
    from frozenbilm_amd import lib

    with pytest.raises(RuntimeError, match="no CPU/eager fallback"):
        lib.load(str(tmp_path / "libfbl.so"))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "frozenbilm_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), os.path.join(dp, f)


def test_gemm_plan_host_query(libpath):
    """fbl_gemm_plan is pure host logic (no launch, no GPU): the shapes of the step that the dispatcher gives to the
    8-phase kernel -- what bench.py's `roofline` attributes to the dominant kernel -- and the ones it does not."""
    from frozenbilm_amd import lib as L

    for shp in [(8512, 6144, 1536), (9024, 4608, 1536), (8512, 1536, 6144), (8512, 1728, 6144), (8512, 1536, 1536),
                (8512, 1536, 4608), (8512, 128100, 1536)]:
        assert L.gemm_plan(*shp) == 8, shp
    for shp in [(8512, 1536, 192), (8512, 192, 1536), (391, 64, 10240), (4100, 3584, 128), (512, 1536, 3072),
                (8512, 1536, 1600)]:
        assert L.gemm_plan(*shp) == 2, shp
    assert L.gemm_plan(8512, 6144, 1536, batch=2) == 2 and L.gemm_plan(8512, 6144, 1536, splitk=4) == 2


def test_adapter_bwd_dw_rejects_bad_arguments_on_the_host(libpath):
    """fbl_adapter_bwd_dw validates its tables before any launch (pure host logic, no GPU needed): group / segment limits,
    the bottleneck padding contract, stride alignment and ranges (include/fbl.h)."""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)
    P = ctypes.c_void_p
    one = (P * 24)(*[0x1000] * 24)  # never dereferenced: every call below fails validation first

    def call(n=1, first=(0, 1), N=128, H=128, A=64, Ap=64, ld=(128, 64, 64, 128), dy=one, first_null=False):
        sf = None if first_null else (ctypes.c_int32 * len(first))(*first)
        lds = [(ctypes.c_int64 * max(n, 1))(*[v] * max(n, 1)) for v in ld]
        return h.fbl_adapter_bwd_dw(n, sf, dy, one, one, one, *lds, N, H, A, Ap, None, None, None, None)

    assert call(n=0) == 0 and call(N=0) == 0  # nothing to do
    assert call(n=17, first=tuple(range(18))) < 0  # more adapters than FBL_ADW_MAX_ADAPTERS
    assert call(first=(1, 2)) < 0          # seg_first[0] must be 0
    assert call(first=(0, 25)) < 0         # more segments than FBL_ADW_MAX_SEGMENTS
    assert call(first=(0, 0)) < 0          # an empty group
    assert call(first_null=True) < 0
    assert call(Ap=96) < 0 and call(Ap=320, A=300) < 0 and call(A=65, Ap=64) < 0  # Ap = A rounded up to 64, <= 256
    assert call(H=100) < 0                 # H % 8
    assert call(ld=(132, 64, 64, 128)) < 0  # stride alignment
    assert call(ld=(64, 64, 64, 128)) < 0   # ld_dy < H
    assert call(ld=(128, 32, 64, 128)) < 0  # ld_z < Ap
    assert call(dy=None) < 0


SHAPE, ALIGN, ARG = -1, -2, -3  # include/fbl.h FBL_ERR_*


def _caller(fn, spec):
    """call(**overrides) -> fn(every argument of `spec`, a list of (name, default) in the order of the C declaration)"""
    names = [n for n, _ in spec]

    def call(**kw):
        assert set(kw) <= set(names), set(kw) - set(names)
        return fn(*[kw.get(n, d) for n, d in spec])

    return call


def test_attention_entry_points_reject_bad_arguments_on_the_host(libpath):
    """The seven disentangled-attention entry points of include/fbl.h validate their arguments, then return 0 for an empty
    problem, and only then touch the HIP runtime: every call below returns before any launch (pointers are never dereferenced,
    no GPU needed).  One fault per call; shape is checked before alignment before the argument rules."""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)
    p, ld = 0x1000, 4608
    dims = [("B", 2), ("S", 64), ("Sp", 64), ("nh", 24)]
    fwd = _caller(h.fbl_disent_attn_fwd, [
        ("q", p), ("ldq", ld), ("k", p), ("ldk", ld), ("v", p), ("ldv", ld), ("pk", p), ("pq", p), ("ldp", 1536), ("relidx", p),
        ("mask", p), ("klen", p), ("border", None), ("scale", 0.125), ("p_drop", 0.0), ("seed", 0), ("seed_dev", None), ("ctx", p),
        ("ldo", 1536), ("lse", p), *dims, ("span2", 512), ("lin_span", 128), ("row0", None), ("psave", None), ("msave", None),
        ("stream", None)])
    ds = _caller(h.fbl_disent_attn_bwd_ds, [
        ("q", p), ("k", p), ("v", p), ("ldq", ld), ("dO", p), ("ldo", 1536), ("pk", p), ("pq", p), ("ldp", 1536), ("relidx", p),
        ("mask", p), ("klen", p), ("border", None), ("lse", p), ("Dv", p), ("scale", 0.125), ("p_drop", 0.0), ("seed", 0),
        ("seed_dev", None), ("dV", p), ("lddv", ld), ("dS", p), ("dST", p), *dims, ("span2", 512), ("lin_span", 128),
        ("row0", None), ("stream", None)])
    dspk = _caller(h.fbl_disent_attn_bwd_dspk, [
        ("psave", p), ("msave", p), ("q", p), ("ldq", ld), ("v", p), ("ldv", ld), ("dO", p), ("ldo", 1536), ("pqx", p), ("klen", p),
        ("border", None), ("lse", p), ("Dv", p), ("scale", 0.125), ("p_drop", 0.0), ("seed", 0), ("seed_dev", None), ("dK", p),
        ("lddk", ld), ("dV", p), ("lddv", ld), ("dS", p), ("dST", p), *dims, ("row0", None), ("stream", None)])
    dq = _caller(h.fbl_disent_attn_bwd_dq, [
        ("dS", p), ("k", p), ("ldk", ld), ("pkx", p), ("klen", p), ("border", None), ("dQ", p), ("lddq", ld), *dims, ("row0", None),
        ("stream", None)])
    shear = _caller(h.fbl_disent_attn_bwd_shear, [
        ("dST", p), ("QT", p), ("y_sh", 64 * 2 * 64), ("y_sb", 64), ("y_sd", 2 * 64), ("PQT", p), ("relidx", p), ("klen", p),
        ("border", None), ("dK", p), ("lddk", ld), ("lin_span", 128), *dims, ("span2", 512), ("row0", None), ("stream", None)])
    ptrs = (ctypes.c_void_p * 2)(p, p)
    pos = _caller(h.fbl_attn_pos_grad, [
        ("neg", 0), ("X", ptrs), ("Y", ptrs), ("ldy", ld), ("dlo", p), ("dcnt", p), ("dcnt_max", 1), ("klen", p), ("row0", None),
        ("out", p), ("E", 2), *dims, ("rcnt", 512), ("stream", None)])
    prep = _caller(h.fbl_attn_bwd_prep, [
        ("q", p), ("ldq", ld), ("pq", p), ("pk", p), ("ldp", 1536), ("dO", p), ("O", p), ("ldo", 1536), ("QT", p), ("PQT", p),
        ("Dv", p), ("relidx", p), ("PQX", p), ("PKX", p), *dims, ("span2", 512), ("row0", None), ("stream", None)])

    # FBL_ERR_SHAPE: S outside 1 .. 512 (fbl_attn_bwd_prep has no upper bound), Sp < S, Sp not a multiple of 64
    for call in (fwd, ds, dspk, dq, shear, pos):
        assert call(S=0, Sp=64) == SHAPE and call(S=513, Sp=576) == SHAPE
        assert call(S=128, Sp=64) == SHAPE and call(S=64, Sp=96) == SHAPE
    assert prep(S=0) == SHAPE and prep(S=128, Sp=64) == SHAPE and prep(S=64, Sp=96) == SHAPE
    assert prep(span2=0) == SHAPE and prep(span2=96) == SHAPE
    assert shear(span2=500) == SHAPE and shear(span2=544) == SHAPE  # span2 % 32, span2 > 512
    assert pos(rcnt=0) == SHAPE and pos(rcnt=1025) == SHAPE

    # FBL_ERR_ALIGN: every stride (8 bf16 elements for what 16-byte loads read, 4 for what 8-byte stores write)
    strides = [(fwd, ("ldq", "ldk", "ldv", "ldp"), ("ldo",)), (ds, ("ldq", "ldo", "ldp"), ("lddv",)),
               (dspk, ("ldq", "ldv", "ldo"), ("lddk", "lddv")), (dq, ("ldk",), ("lddq",)),
               (shear, ("y_sh", "y_sb", "y_sd"), ("lddk",)), (pos, ("ldy",), ()), (prep, ("ldq", "ldp", "ldo"), ())]
    for call, by8, by4 in strides:
        for name in by8:
            assert call(**{name: 1540}) == ALIGN, name  # 1540 % 8 == 4
        for name in by4:
            assert call(**{name: 1538}) == ALIGN, name  # 1538 % 4 == 2
            assert call(**{name: 1540}, B=0) == 0, name  # ... and no more than 4: valid, then empty, so nothing is launched

    # FBL_ERR_ARG
    for call in (fwd, ds):
        assert call(lin_span=-1) == ARG and call(lin_span=257) == ARG  # 2 * lin_span > span2
    for call in (fwd, ds, dspk, dq, shear, pos):
        assert call(row0=p, klen=None) == ARG  # the packed layout is defined by the samples' lengths
    assert fwd(psave=p) == ARG and fwd(msave=p) == ARG and fwd(psave=p, msave=p, lse=None) == ARG
    for name in ("psave", "msave", "q", "v", "dO", "pqx", "lse", "Dv", "dK", "dV", "dS", "dST"):
        assert dspk(**{name: None}) == ARG, name
    for name in ("dS", "k", "pkx", "dQ"):
        assert dq(**{name: None}) == ARG, name
    for name in ("X", "Y", "dlo", "dcnt", "out"):
        assert pos(**{name: None}) == ARG, name
    assert pos(dcnt_max=0) == ARG
    assert pos(X=(ctypes.c_void_p * 2)(p, None)) == ARG and pos(Y=(ctypes.c_void_p * 2)(None, p)) == ARG
    assert prep(relidx=None) == ARG and prep(relidx=None, PQX=None) == ARG and prep(relidx=None, PKX=None) == ARG
    assert prep(Dv=None) == ARG

    # an empty problem: 0, nothing launched
    for call in (fwd, ds, dspk, dq, shear, pos, prep):
        assert call(B=0) == 0 and call(nh=0) == 0
    assert pos(E=0) == 0
