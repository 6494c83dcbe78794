"""CPU: the case table of the grouped adapter weight-gradient kernel (tests/adw_cases.py) really holds the instantiations and
edges it claims to, stays inside the limits the library's binding states (ADW_MAX_ADAPTERS, ADW_MAX_SEGMENTS), and keeps its exact
pass exact; the argument errors fbl_adapter_bwd_dw returns before any HIP call; the layout case tables (tests/layout_cases.py)
have unique names."""
import ctypes as C

import pytest

from tests import adw_cases as AC
from tests import layout_cases as LC

ERR_SHAPE, ERR_ALIGN, ERR_ARG = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib
    from frozenbilm_amd.build import build_lib

    lib.load(build_lib(verbose=False))
    return lib


@pytest.fixture(scope="module")
def cases():
    return AC.cases()


def test_case_names_are_unique(cases):
    names = AC.ids(cases)
    assert len(set(names)) == len(names), names
    for table in LC.TABLES:
        names = LC.ids(table)
        assert len(set(names)) == len(names), names


def test_every_instantiation_full_and_padded(cases):
    for k in (1, 2, 3, 4):
        mine = [c for c in cases if c.Ap // 64 == k]
        assert any(c.A == c.Ap for c in mine), f"adapter_dw_kernel<{2 * k}>: no case with A == Ap"
        assert any(c.A < c.Ap for c in mine), f"adapter_dw_kernel<{2 * k}>: no case with A < Ap"
        assert any(c.random for c in mine), f"adapter_dw_kernel<{2 * k}>: no random-data case"
    assert {c.Ap // 64 for c in cases} == {1, 2, 3, 4}


def test_the_edges_are_in_the_table(cases):
    assert any(c.N % 64 == 0 and c.N == 64 for c in cases), "the non-ragged path at exactly one row tile"
    assert any(c.N % 64 == 0 and c.N > 64 for c in cases), "the non-ragged path over several row tiles"
    assert any(c.N < 64 for c in cases) and any(c.N == 1 for c in cases), "ragged first tile, N = 1"
    assert any(c.N > 64 and c.N % 64 for c in cases), "full tiles followed by a ragged one"
    assert any(c.H % 64 != 0 and c.H > 64 for c in cases), "the clamp of the wide columns in a ragged last tile"
    assert any(c.H == 8 for c in cases), "H == 8: the clamp's limit"
    assert any(c.H % 64 == 0 for c in cases) and any(AC.tiles_h(c) >= 24 for c in cases)
    assert {1, 2, 4} <= {AC.rounds(c) for c in cases}, "rounds of the workgroup -> problem map"
    assert any(2 * c.adapters > 8 and (2 * c.adapters) % 8 for c in cases), "a second round that is not full"
    assert any(2 * c.adapters == 8 for c in cases), "exactly one full round"
    assert any(c.adapters == 1 for c in cases)
    assert any(c.A % 4 != 0 for c in cases), "scalar stores: a4 + 4 > A"
    assert any(c.A % 4 != 0 and c.A > 4 for c in cases) and any(c.A < 4 for c in cases)
    assert any(c.out_offset % 4 != 0 and c.A % 4 == 0 for c in cases), "scalar stores through the pointer alignment alone"
    assert {1, 2, 3} <= {n for c in cases for n in c.seg_counts}
    assert {("dWu",), ("dWd",), ("dbd",), ("dWu", "dWd"), AC.ALL} <= {c.outs for c in cases}
    assert {"tail", "singles", "one"} <= {c.rows for c in cases}
    assert any((c.N, c.H, c.A) == AC.PROD and c.adapters == 16 and c.seg_counts[0] == 2 and c.random for c in cases)
    for c in cases:
        assert c.layout in AC.LAYOUTS and c.rows in AC.ROWS and set(c.outs) <= set(AC.ALL) and c.outs, c.name
        assert len(c.seg_counts) == c.adapters and min(c.seg_counts) >= 1, c.name
        assert c.H % 8 == 0 and 1 <= c.A <= 256 and c.why, c.name
        for s in range(c.n_segments):
            keep = AC.row_keep(c, s)
            assert keep and all(0 <= r < c.N for r in keep) and (c.rows == "all" or len(keep) < c.N), (c.name, s)


def test_the_lora_caller_s_cases(cases):
    lora = [c for c in cases if c.layout == "lora"]
    assert {1, 4, 8, 16} <= {c.A for c in lora} and {511, 40} <= {c.N for c in lora}
    for c in lora:
        assert c.Ap == 64 and "dbd" not in c.outs and c.seg_counts[0] == 3 and c.H == 128 and c.random, c.name
        assert all("dbd" not in c.outs_of(o) for o in range(c.adapters)), c.name


def test_limits_of_the_binding(L, cases):
    assert any(c.n_segments == L.ADW_MAX_SEGMENTS for c in cases), "no case fills the segment table"
    assert any(c.adapters == L.ADW_MAX_ADAPTERS for c in cases), "no case fills the adapter table"
    for c in cases:
        assert c.adapters <= L.ADW_MAX_ADAPTERS and c.n_segments <= L.ADW_MAX_SEGMENTS, c.name


def test_exact_pass_is_exact(cases):
    """integers dy, dz, x in [-2, 2] and z in [0, 3]: a product is at most 6 in magnitude, a sum over segments * N rows at most
    6 * segments * N; below 2^24 every partial sum, in any order, is an integer fp32 holds exactly (the prefill included)"""
    for c in cases:
        assert max(c.seg_counts) * c.N * 6 < 2 ** 24, c.name
        assert c.n_segments * c.N * 6 + AC.PREFILL_MAX < 2 ** 24, c.name


# ------------------------------------------------------------------------------------------------ argument errors
# Only calls that return before the launch (read in adapter_dw.hip: every check sits above hipLaunchKernelGGL); the operand
# tables are read on the host, the pointers in them are never dereferenced.
def _call(h, n, seg_first, N=70, H=128, A=16, Ap=64, ld=(128, 64, 64, 128), ptr=0x1000, tables=True):
    nseg = seg_first[-1] if seg_first else 0
    sf = (C.c_int32 * max(len(seg_first), 1))(*seg_first)
    tab = (C.c_void_p * max(nseg, 1))(*([ptr] * max(nseg, 1)))
    lds = [(C.c_int64 * max(n, 1))(*([v] * max(n, 1))) for v in ld]
    t = tab if tables else None
    return h.fbl_adapter_bwd_dw(n, sf, t, tab, tab, tab, lds[0], lds[1], lds[2], lds[3], N, H, A, Ap, None, None, None, None)


def test_adapter_bwd_dw_rejects_bad_arguments(L):
    h = L.load()
    assert _call(h, 0, [0]) == 0 and _call(h, 1, [0, 1], N=0) == 0                      # empty calls
    assert _call(h, L.ADW_MAX_ADAPTERS + 1, list(range(L.ADW_MAX_ADAPTERS + 2))) == ERR_ARG
    assert _call(h, 1, [0, L.ADW_MAX_SEGMENTS + 1]) == ERR_ARG
    assert _call(h, 1, [1, 2]) == ERR_ARG                                               # seg_first[0] != 0
    assert _call(h, 2, [0, 2, 1]) == ERR_ARG                                            # decreasing
    assert _call(h, 1, [0, 1], Ap=16) == ERR_SHAPE and _call(h, 1, [0, 1], A=65, Ap=64) == ERR_SHAPE
    assert _call(h, 1, [0, 1], A=16, Ap=320) == ERR_SHAPE and _call(h, 1, [0, 1], H=12) == ERR_SHAPE
    assert _call(h, 1, [0, 1], tables=False) == ERR_ARG
    assert _call(h, 1, [0, 1], ld=(132, 64, 64, 128)) == ERR_ALIGN
    assert _call(h, 1, [0, 1], ld=(120, 64, 64, 128)) == ERR_ARG and _call(h, 1, [0, 1], ld=(128, 56, 64, 128)) == ERR_ARG
    assert _call(h, 1, [0, 1], ld=(1 << 24, 64, 64, 128)) == ERR_ARG
    assert _call(h, 1, [0, 1], ptr=None) == ERR_ARG                                      # a NULL operand
