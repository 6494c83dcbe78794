"""The case tables of the layout and staging kernels (frozenbilm_amd/csrc/rowops.hip: transpose_kernel, transpose_batched_kernel,
head_transpose_kernel, im2col3_kernel / col2im3_kernel, embed_gather_kernel, mask_tokens_kernel; csrc/attn_bwd.hip:
attn_bwd_prep_kernel with a packed row layout), run by tests/test_gpu_layout_kernels.py.  All of them move or select values
without arithmetic (col2im3: three additions in a fixed order), so every check is bit equality with the definition."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple


@dataclass(frozen=True)
class Transpose:
    name: str
    rows: int
    cols: int
    rows_pad: int
    ld_in: Optional[int] = None   # row stride of the input (None: cols)
    why: str = ""


@dataclass(frozen=True)
class TransposeBatched:
    name: str
    rows: int
    cols: int
    count: int
    why: str = ""


@dataclass(frozen=True)
class HeadT:
    name: str
    B: int
    S: int
    Sp: int
    nh: int
    why: str = ""


@dataclass(frozen=True)
class Conv3:
    name: str
    B: int
    S: int
    H: int
    why: str = ""


@dataclass(frozen=True)
class Embed:
    name: str
    B: int
    T: int
    Lt: int
    H: int
    V: int
    why: str = ""


@dataclass(frozen=True)
class Prep:
    name: str
    lens: Tuple[int, ...]         # rows of each sample in the packed layout
    S: int
    Sp: int
    nh: int
    span2: int
    why: str = ""


TRANSPOSE = [
    Transpose("tr_1x1", 1, 1, 64, why="one element in one tile"),
    Transpose("tr_64x64", 64, 64, 64, why="exactly one full tile, no padding"),
    Transpose("tr_64x33_pad128", 64, 33, 128, why="a whole tile of padding with no source rows; ragged columns"),
    Transpose("tr_333x200_pad384", 333, 200, 384, why="several tiles both ways, ragged both ways"),
    Transpose("tr_70x8_pad70", 70, 8, 70, why="rows_pad == rows and no multiple of 64: the r < rows_pad bound of the store"),
    Transpose("tr_65x130_ld154", 65, 130, 192, ld_in=130 + 24, why="input row stride > cols"),
]

TRANSPOSE_BATCHED = [
    TransposeBatched("tb_1x1x1", 1, 1, 1, why="one element"),
    TransposeBatched("tb_64x64x3", 64, 64, 3, why="one full tile per matrix"),
    TransposeBatched("tb_70x33x2", 70, 33, 2, why="ragged both ways"),
    TransposeBatched("tb_192x1536x5", 192, 1536, 5, why="an adapter's up weight"),
    TransposeBatched("tb_16x128x24", 16, 128, 24, why="many small matrices"),
]

HEAD_T = [
    HeadT("ht_1_1_64_1", 1, 1, 64, 1, why="one position"),
    HeadT("ht_2_63_64_3", 2, 63, 64, 3, why="one position short of a tile"),
    HeadT("ht_2_64_64_2", 2, 64, 64, 2, why="a full tile, no padding"),
    HeadT("ht_3_65_128_2", 3, 65, 128, 2, why="one position into the second tile"),
    HeadT("ht_2_10_128_1", 2, 10, 128, 1, why="a whole tile beyond S"),
    HeadT("ht_1_266_320_3", 1, 266, 320, 3, why="five tiles"),
]

CONV3 = [
    Conv3("conv_1_1_8", 1, 1, 8, why="both neighbours missing"),
    Conv3("conv_3_2_8", 3, 2, 8, why="every row has one neighbour missing; sample boundaries"),
    Conv3("conv_3_11_128", 3, 11, 128, why="interior rows; sample boundaries"),
    Conv3("conv_2_5_1536", 2, 5, 1536, why="several passes of both column loops (3H/8 = 576 chunks, H/4 = 384 quads)"),
]

EMBED = [
    Embed("emb_1_0_1_4", 1, 0, 1, 4, 1, why="no video rows (vproj = None), one quad per row"),
    Embed("emb_3_4_9_128", 3, 4, 9, 128, 50, why="video rows in front of the text"),
    Embed("emb_2_10_7_1536", 2, 10, 7, 1536, 50, why="three passes of the column loop"),
]

PREP = [Prep("prep_packed", (150, 1, 64, 97), 150, 192, 2, 512, why="packed rows: a full sample, one row, a full tile, a ragged one")]

MASK_N = (1, 255, 257, 32768)       # one thread, one block short of full, a second block with one thread, 128 blocks
MASK_P = (0.0, 0.15, 1.0)
MASK_SEEDS = (42, 0x1234_5678_9ABC_DEF1)

TABLES = (TRANSPOSE, TRANSPOSE_BATCHED, HEAD_T, CONV3, EMBED, PREP)


def ids(cases):
    return [c.name for c in cases]
