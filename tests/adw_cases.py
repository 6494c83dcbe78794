"""The case table of the grouped adapter weight-gradient kernel (frozenbilm_amd/csrc/adapter_dw.hip, fbl_adapter_bwd_dw), shared
by the CPU test of the table itself (tests/test_adw_cases.py) and the GPU tests that run every case against fp64
(tests/test_gpu_adapter_dw.py).

    dWu[H, A] += sum_seg dy^T . z      dWd[A, H] += sum_seg dz^T . x      dbd[A] += sum_seg colsum(dz)

Each case names one launch -- shape, group, segments, operand layout, which outputs exist -- and the branch of the launcher / kernel
it is there for.  What decides a branch, restated from the kernel:

  * Ap / 64 in 1 .. 4 picks adapter_dw_kernel<NT = 2, 4, 6, 8>;
  * a workgroup owns one 64-wide tile column `th` of one problem p = 2 * adapter + which; the grid is dealt in rounds of eight
    problems (p = (slot / tiles_h) * 8 + xcd), so more than four adapters need a second round and p >= 2 * adapters returns early;
  * the wide operand's last tile re-reads the last eight valid columns when H % 64 != 0 (min(h0 + ch * 8, H - 8));
  * N % 64 != 0 takes the ragged load of the last row tile of every segment (narrow rows beyond N read as zero);
  * a store is a 16-byte read-modify-write when four outputs fit and the address is 16-byte aligned, else scalar;
  * the column sums (dbd) ride in tile column 0 of the dWd problem and exist only when dbd is given.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

WT = 64                 # wide columns of a tile (adapter_dw.hip: WT = WI * 32)
XCD_ROUND = 8           # problems dealt per round of the workgroup -> problem map
PREFILL_MAX = 50        # |integer prefill| of the exact pass
ALL = ("dWu", "dWd", "dbd")

# operand layouts
#   "mixed"   odd adapters: dy and dz are column blocks of ONE buffer [dy | dz | 64 sentinel columns] (the folded backward
#             operand), even adapters: dy in its own buffer with ld = H + 64; x: ld = H + 64, z (and an own dz): ld = Ap + 8
#   "lora"    what Engine._lora_products hands in: dy = columns [H, 2H) of an [N, 3H] buffer, z / dz contiguous [N, 64],
#             x contiguous [N, H]
LAYOUTS = ("mixed", "lora")
# rows of dy and dz that are zeroed (the padded operands of the compact backward); z and x keep their values
ROWS = ("all", "tail", "singles", "one")


@dataclass(frozen=True)
class Adw:
    name: str
    N: int
    H: int
    A: int
    adapters: int = 2
    segs: Tuple[int, ...] = ()         # segments per adapter (default: two on the first adapter, one on the others)
    layout: str = "mixed"
    outs: Tuple[str, ...] = ALL        # outputs of the EVEN adapters (the others are None); odd adapters get all three ("mixed")
    out_offset: int = 0                # dWu / dWd are contiguous views at this element offset of a flat buffer
    rows: str = "all"                  # which rows of dy / dz exist (see ROWS)
    random: bool = False               # also run the random-data pass
    why: str = ""

    @property
    def Ap(self) -> int:
        return (self.A + 63) // 64 * 64

    @property
    def seg_counts(self) -> Tuple[int, ...]:
        return self.segs if self.segs else (2,) + (1,) * (self.adapters - 1)

    @property
    def n_segments(self) -> int:
        return sum(self.seg_counts)

    @property
    def K(self) -> int:
        """the longest contraction of the case: rows x segments of one adapter"""
        return max(self.seg_counts) * self.N

    def outs_of(self, o: int) -> Tuple[str, ...]:
        return self.outs if (o % 2 == 0 or self.layout == "lora") else ALL  # (a LoRA site never has a bias gradient)


def tiles_h(c: Adw) -> int:
    return (c.H + WT - 1) // WT


def rounds(c: Adw) -> int:
    """rounds of eight problems the grid is dealt in"""
    return (2 * c.adapters + XCD_ROUND - 1) // XCD_ROUND


def scalar_store(c: Adw) -> bool:
    """some dWu store of the case takes the scalar path (a4 + 4 > A, or a row stride / pointer off 16 bytes)"""
    return c.A % 4 != 0 or c.out_offset % 4 != 0


def row_keep(c: Adw, seg: int):
    """the rows of dy / dz of segment `seg` (counted over the whole case) that exist, as a list of row numbers"""
    N = c.N
    if c.rows == "all":
        return list(range(N))
    if c.rows == "tail":                       # a run of zero rows at the end, of a different length per segment
        return list(range(max(1, N - 9 - 31 * seg)))
    if c.rows == "singles":                    # single zero rows, the first and the last row among them
        return [r for r in range(N) if r not in (0, N - 1) and (r + seg) % 7 != 3]
    if c.rows == "one":                        # all rows but one are zero
        return [(37 * (seg + 1)) % N]
    raise ValueError(c.rows)


PROD = (8512, 1536, 192)  # rows, hidden size and bottleneck of a training step


def cases():
    out = []
    # every instantiation, full (A == Ap) and padded (A < Ap)
    for A in (64, 16, 128, 100, 192, 144, 256, 200):
        out.append(Adw(f"inst_A{A}", 70, 128, A, random=(A % 64 == 0),
                       why=f"adapter_dw_kernel<{(A + 63) // 64 * 2}>, " + ("A == Ap" if A % 64 == 0 else "A < Ap")))
    out += [
        # the narrow store edge
        Adw("store_A18", 70, 128, 18, why="dWu row stride 72 bytes: every other row off 16 bytes; a4 + 4 > A at a4 = 16"),
        Adw("store_A2", 70, 128, 2, why="a4 + 4 > A in the first store of a row; dWu row stride 8 bytes"),
        Adw("store_offset2", 70, 72, 16, out_offset=2, why="dWu / dWd 8-byte aligned: every store takes the scalar path"),
        # the wide edge
        Adw("wide_H8", 70, 8, 16, why="H - 8 = 0: every wide chunk is clamped to column 0"),
        Adw("wide_H64", 70, 64, 16, why="one full tile column, no clamp"),
        Adw("wide_H72", 70, 72, 16, why="second tile column holds 8 columns: clamp to H - 8 = h0"),
        Adw("wide_H200", 70, 200, 16, why="four tile columns, the last one 8 wide"),
        Adw("wide_H1536", 70, 1536, 16, why="24 tile columns"),
    ]
    # rows
    for N, why in ((1, "one row: ragged tile with left = 1"), (63, "N < 64"), (64, "exactly one full tile: the non-ragged path"),
                   (65, "a full tile, then one row"), (128, "two full tiles"), (333, "five full tiles and 13 rows")):
        out.append(Adw(f"rows_N{N}", N, 72, 16, why=why))
    out += [
        # the workgroup -> problem map
        Adw("group_1", 70, 128, 16, adapters=1, why="two problems: six of the eight slots of the round return early"),
        Adw("group_4", 70, 128, 16, adapters=4, why="eight problems: one full round"),
        Adw("group_5", 70, 128, 16, adapters=5, why="a ninth and tenth problem in the second round"),
        Adw("group_16", 130, 200, 192, adapters=16, random=True, why="four rounds of eight problems, four tile columns each"),
        # segments
        Adw("segs_123", 70, 72, 16, adapters=3, segs=(1, 2, 3), why="one, two and three segments per adapter"),
        Adw("segs_24", 70, 72, 16, adapters=16, segs=(2,) * 8 + (1,) * 8, why="the segment table is full"),
        # NULL outputs (on the even adapters; the odd ones write all three)
        Adw("null_only_dWu", 70, 72, 16, outs=("dWu",), why="dWd and dbd NULL"),
        Adw("null_only_dWd", 70, 72, 16, outs=("dWd",), why="dbd NULL while dWd is given: no column sums"),
        Adw("null_only_dbd", 70, 72, 16, outs=("dbd",), why="column sums without the product they ride in"),
        Adw("null_no_dbd", 70, 72, 16, outs=("dWu", "dWd"), why="the LoRA pattern on an adapter shape"),
    ]
    # the LoRA caller: rank inside Ap = 64, dy a column block of the packed [N, 3H] gradient, no bias, three executions of the first site
    for N in (511, 40):
        for r in (1, 4, 8, 16):
            out.append(Adw(f"lora_r{r}_N{N}", N, 128, r, adapters=3, segs=(3, 1, 1), layout="lora", outs=("dWu", "dWd"), random=True,
                           why="Engine._lora_products operands" + (", N = table rows" if N == 511 else ", N < 64")))
    out += [
        Adw("lora_group16", 40, 128, 8, adapters=16, segs=(3,) + (1,) * 15, layout="lora", outs=("dWu", "dWd"), random=True,
            why="a full LoRA group (group independence)"),
        # the padded operands of the compact backward: whole rows of dy and dz are zero
        Adw("compact_tail", 333, 72, 16, rows="tail", why="a run of zero rows at the end of every segment"),
        Adw("compact_singles", 333, 72, 16, rows="singles", why="single zero rows, first and last row included"),
        Adw("compact_one", 333, 72, 16, rows="one", why="all rows but one are zero"),
        # production
        Adw("prod", *PROD, adapters=16, random=True, why="the headline step's group"),
    ]
    return out


def ids(cs):
    return [c.name for c in cs]
