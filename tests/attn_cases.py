"""The case table of the fused disentangled-attention kernels (frozenbilm_amd/csrc/attn_fwd.hip, attn_bwd.hip), shared by the
CPU test of the table and of the float64 references (tests/test_attn_refs.py) and by the GPU test that judges every stage per
element (tests/test_gpu_attn_elementwise.py).

Each case names a grid -- samples, length, heads, the samples' valid positions, the dispatch order, the row layout and the
relative-position map -- and what of the kernels it is there to reach.  The helpers below restate, from the kernels and their
launchers, what decides a branch: the `band` condition of a (query tile, key tile) pair, wg_coord's mapping, the affine span
`lin` each kernel is launched with, the deltas per table row that pick the kernel of fbl_attn_pos_grad.  These are
kernel-correctness shapes, not workload shapes.
"""
from __future__ import annotations

import types
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

FBL_MAP = (256, 512, 256)     # position_buckets, max_relative_positions, att_span: the FrozenBiLM map
COARSE_MAP = (64, 512, 64)    # log buckets from |delta| = 32 on
CLAMPED_MAP = (0, 128, 128)   # no buckets: clamp(delta + span, 0, 2 span - 1)

SCALE = 1.0 / (64 * 3) ** 0.5
P_DROPS = (0.0, 0.1)
SEED = 0x5EEDA77


@dataclass(frozen=True)
class Case:
    B: int
    S: int
    nh: int
    klen: Optional[Tuple[int, ...]]   # valid positions per sample passed to the kernels (None: the dense grid, no tile skipping)
    holes: Tuple[Tuple[int, int, int], ...] = ()   # (sample, first, last + 1): masked positions inside a sample
    tail: Tuple[Tuple[int, int], ...] = ()          # (sample, first masked position): a masked tail without a klen
    border: bool = False              # samples dispatched longest first
    packed: bool = False              # activation rows without the padding rows (row0)
    cmap: Tuple[int, int, int] = FBL_MAP
    reaches: str = ""


CASES = {
    "s1": Case(2, 1, 2, None, reaches="smallest accepted grid"),
    "s37": Case(2, 37, 2, None, holes=((1, 1, 3),), tail=((0, 32),), reaches="one tile, Sp > S, identity band only"),
    "s64": Case(1, 64, 1, None, reaches="S == Sp, exactly one tile"),
    "s130": Case(2, 130, 2, (125, 130), reaches="first tile pair outside the band (tile distance 2); first log buckets"),
    "s266x": Case(4, 266, 2, (266, 1, 20, 100), border=True,
                  reaches="nh*B % 8 == 0 mapping; query tiles beyond klen; 3 deltas per table row"),
    "s266p": Case(4, 266, 2, (100, 266, 20, 1), packed=True, reaches="the PACKED instantiations of every kernel"),
    "s512": Case(2, 512, 1, (512, 200), reaches="S == Sp == 512, up to 6 deltas per row, window clamp at the table ends"),
    "coarse": Case(1, 266, 2, None, cmap=COARSE_MAP,
                   reaches="lin = 32: almost every pair gathered through the index table; prefix-difference pos_grad kernel"),
    "clamped": Case(1, 300, 2, None, cmap=CLAMPED_MAP,
                    reaches="every delta beyond the span on the two edge rows; lin = 0 forward"),
}
RECOMPUTE_CASES = ("s130", "s266x", "s266p", "s512", "coarse", "clamped")


# ------------------------------------------------------------------------------------------------ host formulas
def cfg_of(case: Case):
    pb, mr, span = case.cmap
    return types.SimpleNamespace(position_buckets=pb, max_rel=mr, att_span=span)


def span2_of(case: Case) -> int:
    return 2 * case.cmap[2]


def pad64(S: int) -> int:
    return (S + 63) // 64 * 64


def relidx_np(case: Case) -> np.ndarray:
    from frozenbilm_amd.model.relpos import rel_index_vector

    pb, mr, span = case.cmap
    return np.asarray(rel_index_vector(case.S, pb, mr, span)).astype(np.int16)


def lin_fwd(case: Case) -> int:
    """affine span the forward is launched with (engine: identity buckets only; a clamped table runs without)"""
    pb, _, span = case.cmap
    return min(pb // 2, span) if pb > 0 else 0


def lin_bwd(case: Case) -> Tuple[int, int]:
    """(lin of recompute kernel A, lin of the shear pass) as attn_bwd.disent_attn_bwd sets them"""
    pb, _, span = case.cmap
    lin = pb // 2 if pb > 0 else span - 1
    return (min(lin, span) if pb > 0 else 0), lin


def band(i0: int, j0: int, lin: int) -> bool:
    """attn_fwd.hip / attn_bwd.hip kernel A: every pair of the 64 x 64 tile lies inside the identity band"""
    return max(abs(i0 - (j0 + 63)), abs(i0 + 63 - j0)) < lin


def xcd_mapping(case: Case) -> bool:
    """attn_common.h wg_coord: the XCD-aware workgroup mapping is taken iff (nh * B) & 7 == 0"""
    return ((case.nh * case.B) & 7) == 0


def lengths(case: Case):
    """(kl, lens): last valid position + 1 of every sample, and the number of activation rows each sample has"""
    kl = list(case.klen) if case.klen is not None else [case.S] * case.B
    return kl, (kl if case.packed else [case.S] * case.B)


def visited_tiles(case: Case, b: int):
    """(query tiles, key tiles) the full-grid kernels visit for sample b: all of them without klen, else those below it"""
    nt = pad64(case.S) // 64
    if case.klen is None:
        return nt, nt
    n = (case.klen[b] + 63) // 64
    return n, n


def mask_np(case: Case) -> np.ndarray:
    kl, _ = lengths(case)
    m = np.zeros((case.B, case.S), dtype=np.int32)
    for b in range(case.B):
        m[b, :kl[b]] = 1
    for b, lo, hi in case.holes:
        m[b, lo:hi] = 0
    for b, lo in case.tail:
        m[b, lo:] = 0
    return m


def delta_ranges_np(case: Case):
    """(rmin, dlo, dcnt) of attn_bwd._delta_ranges on the host: table row rmin + r collects the deltas [dlo[r], dlo[r] + dcnt[r])"""
    rv = relidx_np(case).astype(np.int64)
    S = case.S
    rmin, rcnt = int(rv[0]), int(rv[-1]) - int(rv[0]) + 1
    first = np.searchsorted(rv, np.arange(rmin, rmin + rcnt), side="left")
    last = np.searchsorted(rv, np.arange(rmin, rmin + rcnt), side="right")
    return rmin, first - (S - 1), last - first


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(name: str, dev, *, backward: bool):
    """Deterministic bf16 inputs of a case on `dev`: unit variance for the forward checks, x 0.5 for the backward ones (as
    test_gpu_kernels.py does).  qkv [rows, 3H] and dctx [rows, H] follow the case's row layout; mask / lse keep [B, S]."""
    c = CASES[name]
    H = c.nh * 64
    span2 = span2_of(c)
    kl, lens = lengths(c)
    row0 = [0]
    for n in lens:
        row0.append(row0[-1] + n)
    g = torch.Generator(device="cpu").manual_seed(4000 + c.S + 17 * sorted(CASES).index(name))
    sc = 0.5 if backward else 1.0
    qkv = (torch.randn(row0[-1], 3 * H, generator=g) * sc).to(torch.bfloat16)
    pqk = (torch.randn(span2, 2 * H, generator=g) * sc).to(torch.bfloat16)
    dctx = torch.randn(row0[-1], H, generator=g).to(torch.bfloat16)
    klen_t = torch.tensor(kl, dtype=torch.int32) if c.klen is not None else None
    border = None
    if c.border:
        border = torch.argsort(klen_t, descending=True, stable=True).to(torch.int32)

    def d(t):
        return None if t is None else t.to(dev).contiguous()

    return types.SimpleNamespace(
        name=name, case=c, B=c.B, S=c.S, Sp=pad64(c.S), nh=c.nh, H=H, span2=span2, scale=SCALE, kl=kl, lens=lens, row0_host=row0,
        qkv=d(qkv), pqk=d(pqk), dctx=d(dctx), mask=d(torch.from_numpy(mask_np(c))), relidx=d(torch.from_numpy(relidx_np(c))),
        klen=d(klen_t), border=d(border), row0=d(torch.tensor(row0, dtype=torch.int32)) if c.packed else None,
        cfg=cfg_of(c), lin_fwd=lin_fwd(c))
