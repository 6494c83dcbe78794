"""The case table of the fused BERT attention (frozenbilm_amd/csrc/mha.hip: fbl_mha_fwd, fbl_mha_bwd and the packed *_rows
entries), shared by the CPU test of the references (tests/test_mha_refs.py) and the GPU test that judges every element
(tests/test_gpu_mha_elementwise.py).

A case names a grid -- samples, length, heads -- the key mask of every sample, and how the operands lie in memory.  Heads are
independent, so nh stays small: the float64 [B, nh, S, S] tensors of the reference must stay cheap.  These are
kernel-correctness shapes, not workload shapes: what decides a path in mha.hip is the number of 64-key tiles, a partial last
tile, a tile without a valid key in front of valid ones (the online softmax wipes it with alpha = exp2(-14427) = 0), a sample
without any valid key (every score carries the -10000 bias: lse ~ -1e4), the tiles beyond klen (skipped), wg_coord's mapping
((nh * B) & 7) and the six row strides.

Every case runs at p_drop 0 and 0.1, with dO random in every row.
"""
from __future__ import annotations

import math
import types
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch

BF16 = torch.bfloat16
SCALE = 1.0 / math.sqrt(64)
P_DROPS = (0.0, 0.1)
SEED = 0x5EEDB27          # the dropout seed of every run
DATA_SEED = 20240         # + a per-case offset: the generator of q, k, v and dO
SENT_BF16 = 0x7FA5        # NaN bit pattern of the sentinel prefill (tests/attn_refs.py)
GUARD_ROWS = 8


def _inputs_masks(S):
    """the four masks of tests/test_gpu_mha._inputs: full; ragged with zeros at keys 1..3; no valid key; short"""
    m = torch.ones(4, S, dtype=torch.int32)
    m[1, max(1, (2 * S) // 3):] = 0
    m[1, 1:min(S, 4)] = 0
    m[2] = 0
    m[3, max(1, S // 5):] = 0
    return m


def _prefix_masks(S, klens):
    m = torch.zeros(len(klens), S, dtype=torch.int32)
    for b, n in enumerate(klens):
        m[b, :n] = 1
    return m


def _late_masks(S):
    m = torch.ones(4, S, dtype=torch.int32)
    m[1, :70] = 0                       # the whole leading key tile masked, valid keys after it
    m[2, 61:64] = 0                     # interior zeros on both sides of key 64 (the tile edge), key 64 itself valid
    m[2, 65:68] = 0
    m[3, 26:] = 0
    return m


def _hot_masks(S):
    m = torch.ones(2, S, dtype=torch.int32)
    m[1, 177:] = 0
    return m


def _strided_masks(S):
    m = torch.ones(2, S, dtype=torch.int32)
    m[1, 86:] = 0
    m[1, 1:4] = 0
    return m


@dataclass(frozen=True)
class Case:
    B: int
    S: int
    nh: int
    masks: Callable[[int], torch.Tensor]
    qk_scale: float = 1.0              # q and k are multiplied by it (peaked scores)
    strided: bool = False              # every operand in a buffer of its own, with its own row stride and guard columns
    reaches: str = ""


CASES = {
    "s1": Case(2, 1, 2, lambda S: _prefix_masks(S, (1, 0)), reaches="P = 1: dS is nothing but the cancellation residue"),
    "s37": Case(4, 37, 3, _inputs_masks, reaches="one partial tile; interior zeros; a sample without a valid key"),
    "s64": Case(3, 64, 2, lambda S: _prefix_masks(S, (64, 63, 1)), reaches="an exact tile"),
    "s65": Case(3, 65, 2, lambda S: _prefix_masks(S, (65, 64, 0)), reaches="a second tile that holds one key"),
    "s129late": Case(4, 129, 3, _late_masks, reaches="a wholly masked leading tile; zeros on both sides of a tile edge"),
    "s266": Case(4, 266, 3, _inputs_masks, reaches="five tiles, a partial last one, odd head count, longest-first order"),
    "s266hot": Case(2, 266, 2, _hot_masks, qk_scale=3.0, reaches="peaked softmax: m_run moves between tiles"),
    "s512": Case(2, 512, 2, lambda S: _prefix_masks(S, (512, 341)), reaches="the maximum S, 8 tiles"),
    "s129strided": Case(2, 129, 12, _strided_masks, strided=True,
                        reaches="eight buffers, eight row strides, (nh * B) & 7 == 0 mapping"),
}
CPU_CASES = tuple(n for n, c in CASES.items() if c.S <= 129)

# row strides of the strided case (H = 768): multiples of 8 for what the kernels load 16 bytes at a time, of 4 only for what
# they store 8 bytes at a time; none equals H or 3H and no two are equal
STRIDES = dict(q=776, k=784, v=800, dO=808, ctx=796, dQ=772, dK=780, dV=788)
# fbl_attn_rowdot takes ONE row stride for dO and ctx, fbl_mha_bwd_rows one each (ctx then needs a multiple of 8): the strided
# case also runs the packed entries on its rows (row0 = b S), with the ctx bits in a buffer of this stride
STRIDE_O_ROWS = 816

# packed rows (fbl_mha_*_rows): rows per sample.  plen > klen on sample 1, the sample without a valid key keeps all its rows
ROWS_CASES = {"s37": (37, 30, 37, 7), "s266": (266, 200, 266, 64)}


def pad64(S: int) -> int:
    return (S + 63) // 64 * 64


def klen_of(mask: torch.Tensor):
    """last valid key + 1 of every sample (0: no valid key), as tests/test_gpu_mha._klen"""
    S = mask.shape[1]
    return [int(v) for v in (mask.cpu() * torch.arange(1, S + 1, dtype=torch.int32)).amax(1)]


def key_tiles(kl: int, S: int, pl: Optional[int] = None) -> int:
    """mha.hip key_limit: the 64-key tiles a sample's workgroups visit -- [0, klen) rounded up; every tile of the sample when it
    has no valid key (the reference then softmaxes over all keys)"""
    lim = kl if kl > 0 else S
    if pl is not None:
        lim = min(lim, pl)
    return (lim + 63) // 64


def xcd_mapping(case: Case) -> bool:
    """attn_common.h wg_coord: the XCD-aware workgroup mapping is taken iff (nh * B) & 7 == 0"""
    return ((case.nh * case.B) & 7) == 0


def sentinel_rows(rows, cols, dev, dtype=BF16):
    """[rows + GUARD_ROWS, cols] filled with the sentinel; the caller uses [:rows, :H]"""
    assert dtype == BF16
    full = torch.empty(rows + GUARD_ROWS, cols, dtype=dtype, device=dev)
    full.view(torch.int16).fill_(SENT_BF16)
    return full


def make_inputs(name: str, dev="cpu", plen: Optional[Tuple[int, ...]] = None):
    """The operands of a case as 2-D bf16 row views [rows, H] (q, k, v, dO) plus mask, klen, border and the row layout.
    Default layout: q | k | v fused in one [B*S, 3H] buffer (row stride 3H, as the fused QKV GEMM leaves it), dO [B*S, H].
    strided: eight separate buffers (STRIDES), sentinel guard columns between the rows.
    plen: the packed-row layout -- sample b has the rows [row0[b], row0[b] + plen[b]) and nothing else; the values of a row are
    those of the padded grid's row (b, s)."""
    c = CASES[name]
    B, S, nh = c.B, c.S, c.nh
    H = nh * 64
    g = torch.Generator().manual_seed(DATA_SEED + list(CASES).index(name))
    qkv = torch.randn(B * S, 3 * H, generator=g) * 0.7
    qkv[:, :2 * H] *= c.qk_scale
    qkv = qkv.to(BF16)
    dO = torch.randn(B * S, H, generator=g).to(BF16)
    mask = c.masks(S)
    assert mask.shape == (B, S)
    kl = klen_of(mask)
    io = types.SimpleNamespace(name=name, case=c, B=B, S=S, Sp=pad64(S), nh=nh, H=H, scale=SCALE, kl=kl, strided=c.strided)
    io.mask = mask.to(dev)
    io.klen = torch.tensor(kl, dtype=torch.int32, device=dev)
    io.border = torch.argsort(io.klen.cpu(), descending=True, stable=True).to(torch.int32).to(dev)
    io.lens = list(plen) if plen is not None else [S] * B
    io.packed = plen is not None
    if plen is not None:
        assert not c.strided
        assert all(kl[b] <= plen[b] <= S and (kl[b] > 0 or plen[b] == S) for b in range(B)), "see ROWS_CASES"
    io.row0_host = [sum(io.lens[:b]) for b in range(B + 1)]
    io.row0 = torch.tensor(io.row0_host, dtype=torch.int32, device=dev) if plen is not None else None
    io.rows = io.row0_host[-1]
    sel = torch.cat([b * S + torch.arange(io.lens[b]) for b in range(B)])
    io.sel = sel.to(dev)
    if c.strided:
        io.ld = dict(STRIDES)
        for i, nm in enumerate(("q", "k", "v")):
            buf = sentinel_rows(io.rows, io.ld[nm], dev)
            buf[:io.rows, :H] = qkv[:, i * H:(i + 1) * H].to(dev)
            setattr(io, nm, buf[:io.rows, :H])
            setattr(io, nm + "_buf", buf)
        buf = sentinel_rows(io.rows, io.ld["dO"], dev)
        buf[:io.rows, :H] = dO.to(dev)
        io.dO, io.dO_buf = buf[:io.rows, :H], buf
        # the same data in the default layout: the strided call must return its bits
        io.fused = make_fused(qkv, dO, io, dev)
    else:
        f = make_fused(qkv[sel], dO[sel], io, dev)
        io.ld = dict(q=3 * H, k=3 * H, v=3 * H, dO=H, ctx=H, dQ=3 * H, dK=3 * H, dV=3 * H)
        io.q, io.k, io.v, io.dO = f.q, f.k, f.v, f.dO
        io.qkv_buf, io.dO_buf = f.qkv_buf, f.dO_buf
    return io


def make_fused(qkv, dO, io, dev):
    rows, H = qkv.shape[0], io.H
    f = types.SimpleNamespace()
    f.qkv_buf = sentinel_rows(rows, 3 * H, dev)
    f.qkv_buf[:rows] = qkv.to(dev)
    f.dO_buf = sentinel_rows(rows, H, dev)
    f.dO_buf[:rows] = dO.to(dev)
    f.q, f.k, f.v = (f.qkv_buf[:rows, i * H:(i + 1) * H] for i in range(3))
    f.dO = f.dO_buf[:rows]
    return f


def input_guards_intact(io) -> bool:
    """no launch wrote into an input buffer: the guard rows and guard columns still hold the sentinel"""
    ok = True
    bufs = [getattr(io, n) for n in ("q_buf", "k_buf", "v_buf", "dO_buf", "qkv_buf") if hasattr(io, n)]
    for buf in bufs:
        bits = buf.view(torch.int16)
        ok &= bool((bits[io.rows:] == SENT_BF16).all())
        if buf.shape[1] not in (io.H, 3 * io.H):
            ok &= bool((bits[:io.rows, io.H:] == SENT_BF16).all())
    return ok
