"""CPU: include/fbl_qrows.h, lib.QROWS_SIGNATURES and the built library agree on the selected-query-row attention entry points,
they validate their arguments on the host before any launch, and the host plan of the selected rows matches brute force."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fbl_disent_attn_fwd_qrows", "fbl_disent_attn_bwd_qrows", "fbl_disent_attn_bwd_qrows_ws_bytes"}


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

    decl = declared_functions("fbl_qrows.h")
    assert set(decl) == NAMES == set(lib.QROWS_SIGNATURES), set(decl) ^ set(lib.QROWS_SIGNATURES)
    for name, (ret, nargs) in decl.items():
        res, argtypes = lib.QROWS_SIGNATURES[name]
        assert len(argtypes) == nargs, name
        assert {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[ret] is res, name
    assert not NAMES & set(lib.SIGNATURES) and not NAMES & set(lib.MHA_SIGNATURES)
    assert len(declared_functions("fbl.h")) == len(lib.SIGNATURES) == 47  # include/fbl.h keeps its declarations


def test_library_exports_them_at_abi_9(libpath):
    from frozenbilm_amd import build, lib

    h = ctypes.CDLL(libpath)
    for name in NAMES:
        assert hasattr(h, name), name
    assert lib.load(libpath).fbl_abi_version() == lib.ABI_VERSION == 9
    hdr = os.path.join(ROOT, "include", "fbl_qrows.h")
    assert build._deps_mtime() >= os.path.getmtime(hdr)


def test_bad_arguments_are_refused_on_the_host(libpath):
    """NULL rseg / rpos / klen, S in {0, 513}, a misaligned stride, p_drop in {1, -0.5} and a negative R are refused before any
    launch, R = 0 returns 0: the pointers are never dereferenced (no GPU needed)."""
    from frozenbilm_amd import lib as L

    h = L.load(libpath)
    p, H = 0x1000, 128

    def fwd(rseg=p, rpos=p, klen=p, S=64, ldq=H, p_drop=0.0, R=4, span2=512):
        return h.fbl_disent_attn_fwd_qrows(p, ldq, rseg, rpos, R, p, 3 * H, p, 3 * H, p, p, 2 * H, p, p, klen, None, 0.07, p_drop,
                                           0, None, p, H, p, 2, S, 64 if S <= 64 else 576, 2, span2, None)

    def bwd(rseg=p, rpos=p, klen=p, S=64, ldq=H, p_drop=0.0, R=4, span2=512, ws=p, ws_bytes=1 << 30):
        return h.fbl_disent_attn_bwd_qrows(p, ldq, rseg, rpos, R, p, 3 * H, p, 3 * H, p, p, 2 * H, p, p, klen, None, p, H, p, H, p,
                                           0.07, p_drop, 0, None, p, H, p, 3 * H, p, 3 * H, p, p, 0, 512, ws, ws_bytes, 2, S,
                                           64 if S <= 64 else 576, 2, span2, None)

    for call in (fwd, bwd):
        assert call(rseg=None) == call(rpos=None) == call(klen=None) == -3
        assert call(S=0) == call(S=513) == -1
        assert call(span2=513) == -1
        assert call(ldq=H + 4) == -2
        assert call(p_drop=1.0) == call(p_drop=-0.5) == -3
        assert call(R=-1) == -3
        assert call(R=0) == 0
    assert bwd(ws=None) == -3 and bwd(ws_bytes=16) == -3  # a workspace that is missing or too small
    assert h.fbl_disent_attn_bwd_qrows_ws_bytes(5, 64, 2) == 2 * 2 * 5 * 64 * 2 + 5 * 8
    assert h.fbl_disent_attn_bwd_qrows_ws_bytes(0, 64, 2) == 0


# ------------------------------------------------------------------------------------------------ the row plan
def _brute(rows, B, S, inv):
    order = sorted(range(len(rows)), key=lambda i: rows[i] // S)  # Python's sort is stable
    grid = [rows[i] for i in order]
    rseg = [0] * (B + 1)
    for r in grid:
        rseg[r // S + 1] += 1
    rseg = list(np.cumsum(rseg))
    return order, grid, rseg, [r % S for r in grid], [inv[r] if inv is not None else r for r in grid]


B_, S_ = 4, 7
PACKED_INV = []
for _b, _n in enumerate((7, 3, 5, 1)):  # a packed layout: sample b keeps its first n rows
    PACKED_INV += [sum((7, 3, 5, 1)[:_b]) + s if s < _n else -1 for s in range(S_)]

CASES = {
    "unsorted": [20, 3, 15, 0, 22, 1],
    "sample_without_rows": [27, 2, 21, 5],
    "all_rows_of_a_sample": list(range(7, 14)) + [0],
    "duplicates": [9, 9, 2, 9, 23, 2],
    "empty": [],
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("packed", [False, True])
def test_row_plan_matches_brute_force(case, packed):
    from frozenbilm_amd.row_plan import plan_query_rows

    rows = CASES[case]
    if packed:
        rows = [r for r in rows if PACKED_INV[r] >= 0] if case != "empty" else rows
    inv = PACKED_INV if packed else None
    pl = plan_query_rows(torch.tensor(rows, dtype=torch.int32), B_, S_, inv=torch.tensor(inv) if packed else None)
    order, grid, rseg, rpos, krows = _brute(rows, B_, S_, inv)
    assert pl.R == len(rows)
    assert pl.order.tolist() == order and pl.grid.tolist() == grid
    assert pl.rseg.dtype == torch.int32 and pl.rseg.tolist() == rseg
    assert pl.rpos.dtype == torch.int32 and pl.rpos.tolist() == rpos
    assert pl.krows.tolist() == krows
    # grouped by sample, the position is the one inside the sample, and the inverse permutation restores the caller's order
    samples = [g // S_ for g in pl.grid.tolist()]
    assert samples == sorted(samples)
    for b in range(B_):
        assert all(s == b for s in samples[rseg[b]:rseg[b + 1]])
    assert pl.grid[pl.back].tolist() == rows
    assert (pl.grid == torch.div(pl.grid, S_, rounding_mode="floor") * S_ + pl.rpos).all()
