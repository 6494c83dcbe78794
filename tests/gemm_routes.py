"""The route table of the NT GEMM (frozenbilm_amd/csrc/gemm.hip plan_gemm), shared by the planner's CPU tests
(tests/test_gemm_plan.py) and the GPU tests that run every route (tests/test_gpu_gemm_routes.py).

Each Route names one call of an entry point -- shape, options, the strides the GPU test allocates -- and the launches
fbl_gemm_plan_launches must report for it on a 256-CU device, in launch order: (kernel, row0, rows, on_aux).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

PLAIN, ADAPTER_DOWN, DENSE, TAIL = 0, 1, 2, 3  # include/fbl.h FBL_GEMM_ENTRY_*
ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_GRAD = 0, 1, 2, 3
AUX_NONE, AUX_ADD_F32, AUX_ADD_BF16, AUX_MUL_DGELU, AUX_MUL_POS, AUX_MUL_BF16 = 0, 1, 2, 3, 4, 5

KERNELS = ("G8_256", "G8_224", "G8_128", "G8_SPLITK", "T2_256", "T2_224", "T2_128", "T2_64_RING", "T2_128_SPLITK")
ACT_NAMES = {ACT_NONE: "NONE", ACT_GELU: "GELU", ACT_RELU: "RELU", ACT_GELU_GRAD: "GELU_GRAD"}
AUX_NAMES = {AUX_NONE: "NONE", AUX_ADD_F32: "ADD_F32", AUX_ADD_BF16: "ADD_BF16", AUX_MUL_DGELU: "MUL_DGELU",
             AUX_MUL_POS: "MUL_POS", AUX_MUL_BF16: "MUL_BF16"}


@dataclass(frozen=True)
class Route:
    name: str
    entry: int
    M: int
    N: int            # columns of the GEMM (dense + adapter-down: N1 + A; adapter tail: H)
    K: int            # (adapter tail: A)
    expect: Tuple[Tuple[str, int, int, bool], ...]
    act: int = ACT_NONE
    aux: int = AUX_NONE
    outs: Tuple[str, ...] = ("out_f32",)  # plain: out_f32 / out_bf16 / out_pre; dense: y_f32 (out_f32) / y_bf16 (out_bf16)
    bias: bool = True
    rowscale: bool = False
    alpha: float = 1.0
    seg_n: int = 0    # dense + adapter-down: N1
    drop: bool = False
    splitk: int = 1
    ws: Optional[int] = None  # split-K workspace floats (None: no workspace pointer)
    aux_stream: bool = False
    r_norm: bool = False
    splitk_out: int = 1       # expected GemmPlan splitk / k8_per / fold
    k8_per: int = 0
    fold: bool = False
    note: str = ""

    @property
    def id(self):
        return self.name

    # ---- the layout the GPU test allocates (and the query is given): operand rows padded by 16 columns, outputs by
    # 8 columns past N rounded up to 8 (so every output has ldc > N and a guard band on the right)
    @property
    def lda(self):
        return self.K + 16

    @property
    def ldb(self):
        return self.K + 16

    @property
    def ldc(self):
        return ((self.seg_n if self.entry == DENSE else self.N) + 7) // 8 * 8 + 8  # (dense: y's row stride)

    @property
    def ld_aux(self):
        if self.entry == DENSE:
            return (self.N - self.seg_n + 7) // 8 * 8 + 8  # ldz
        if self.entry == TAIL:
            return (self.N + 7) // 8 * 8 + 8               # ldx
        return self.ldc if self.aux != AUX_NONE else 0

    def opts(self, aux_stream=None):
        o = list(self.outs) if self.entry in (PLAIN, DENSE) else []
        if self.bias:
            o.append("bias")
        if self.rowscale:
            o.append("rowscale")
        if self.aux != AUX_NONE:
            o.append("aux")
        if self.drop:
            o.append("dropout")
        if self.ws is not None:
            o.append("ws")
        if self.aux_stream if aux_stream is None else aux_stream:
            o.append("aux_stream")
        if self.r_norm:
            o.append("r_norm")
        return tuple(o)

    def query(self, lib, n_cu=256, aux_stream=None):
        """(code, plan) of fbl_gemm_plan_launches for this call"""
        return lib.gemm_plan_launches(self.entry, self.M, self.N, self.K, lda=self.lda, ldb=self.ldb, ldc=self.ldc,
                                      ld_aux=self.ld_aux, seg_n=self.seg_n, act=self.act, aux_kind=self.aux,
                                      opts=self.opts(aux_stream), splitk=self.splitk, ws_floats=self.ws or 0, n_cu=n_cu)


def one(k, M):
    return ((k, 0, M, False),)


def _plain(name, M, N, K, kernel, **kw):
    return Route(name, PLAIN, M, N, K, kw.pop("expect", None) or one(kernel, M), **kw)


F32, BF16, PRE = ("out_f32",), ("out_bf16",), ("out_bf16", "out_pre")

ROUTES = [
    # ---- 8-phase 256x256: every instantiated epilogue (gemm8_supports(., ., 256)); 238 tiles in one round
    _plain("g8_256_none", 4100, 3584, 256, "G8_256", outs=("out_f32", "out_bf16"), rowscale=True, alpha=1.25),
    _plain("g8_256_gelu", 4100, 3584, 256, "G8_256", act=ACT_GELU, outs=PRE, rowscale=True),
    _plain("g8_256_gelu_grad", 4100, 3584, 256, "G8_256", act=ACT_GELU_GRAD, outs=PRE),
    _plain("g8_256_add_f32", 4100, 3584, 256, "G8_256", aux=AUX_ADD_F32, alpha=0.5),
    _plain("g8_256_add_bf16", 4100, 3584, 256, "G8_256", aux=AUX_ADD_BF16, outs=BF16, bias=False),
    _plain("g8_256_mul_bf16", 4100, 3584, 256, "G8_256", aux=AUX_MUL_BF16, outs=BF16, bias=False),
    _plain("g8_256_mul_dgelu", 4100, 3584, 256, "G8_256", aux=AUX_MUL_DGELU, outs=BF16, bias=False),
    # ragged last tile column (3500 = 13 x 256 + 172) and row (4100 = 16 x 256 + 4)
    _plain("g8_256_ragged_n", 4100, 3500, 256, "G8_256", outs=("out_f32", "out_bf16")),
    # a few hundred rows against a very wide N (the vocabulary GEMM of the loss on the labelled rows)
    _plain("g8_256_wide_n", 691, 16500, 256, "G8_256", outs=BF16),
    # ---- 8-phase 224x256 (r224: fewer rounds x tile area than 256x256) -- NONE and ADD_F32
    _plain("g8_224_none", 8512, 1536, 384, "G8_224", outs=("out_f32", "out_bf16")),
    _plain("g8_224_add_f32", 8512, 1536, 384, "G8_224", aux=AUX_ADD_F32, alpha=1.25),
    _plain("g8_224_ragged", 4100, 2052, 256, "G8_224", outs=F32, note="r224 (4100 = 18 x 224 + 68); ragged column tile"),
    # the single_launch window: 36 x 18 = 648 tiles of 256 rows, 648 % 256 = 136 in [96, 192] -> one 224-row launch
    _plain("single_launch_qkv", 9024, 4608, 1536, "G8_224", outs=BF16),
    # GELU has no 224-row instance: r224 holds, the launch stays on 256-row tiles
    _plain("g8_gelu_r224_to_256", 8512, 1536, 384, "G8_256", act=ACT_GELU, outs=PRE),
    # ---- 8-phase 128x256: the cost model's G8_128 side (N = 1536 dX GEMMs at packed / small-batch row counts)
    _plain("g8_128_none", 1500, 1536, 1536, "G8_128", outs=("out_f32", "out_bf16")),
    _plain("g8_128_add_f32", 1500, 1536, 1536, "G8_128", aux=AUX_ADD_F32, alpha=0.5),
    _plain("g8_128_packed", 5322, 1536, 6144, "G8_128", outs=BF16, bias=False),
    _plain("g8_128_ragged", 1025, 1279, 512, "G8_128", outs=F32, note="M = 8 x 128 + 1, N = 5 x 256 - 1"),
    # ... and its other side: same rows at K = 256 -> 2-stage 128x128
    _plain("g8_128_rejected", 1500, 1536, 256, "T2_128", outs=F32),
    # ---- whole rounds + remainder rows (rem < 2/3 of the CUs): 34 x 24 = 816 tiles, 48 left
    _plain("split_ring_rem", 8512, 6144, 1536, None, outs=BF16,
           expect=(("T2_64_RING", 8192, 320, False), ("G8_256", 0, 8192, False))),
    _plain("split_ring_rem_aux", 8512, 6144, 1536, None, outs=BF16, aux_stream=True,
           expect=(("T2_64_RING", 8192, 320, True), ("G8_256", 0, 8192, False))),
    _plain("split_t2_128_rem", 8892, 6144, 256, None, outs=F32, aux_stream=True,
           expect=(("T2_128", 8192, 700, True), ("G8_256", 0, 8192, False))),
    # whole rounds that fall back: odd nk (5) -> 2-stage 256x256; whole-round rows too short for big tiles -> 128x128
    _plain("split_rounds_t2_256", 4100, 4608, 320, None, outs=F32,
           expect=(("T2_64_RING", 3584, 516, False), ("T2_256", 0, 3584, False))),
    _plain("split_rounds_t2_128", 2048, 8448, 256, None, outs=F32,
           expect=(("T2_64_RING", 1792, 256, False), ("T2_128", 0, 1792, False))),
    # ---- the 8-phase kernel's K limits: nk < 4 and odd nk fall back to the 2-stage big tiles
    _plain("t2_256_nk2", 4100, 3584, 128, "T2_256", outs=("out_f32", "out_bf16")),
    _plain("t2_256_nk3", 4100, 3584, 192, "T2_256", outs=F32),
    _plain("t2_224_nk3", 8512, 1536, 192, "T2_224", outs=("out_f32", "out_bf16")),
    _plain("t2_224_odd", 4100, 2052, 320, "T2_224", outs=F32, note="nk = 5"),
    # ---- 2-stage 128x128: every epilogue of launch_one
    _plain("t2_128_none", 300, 256, 128, "T2_128", outs=("out_f32", "out_bf16"), rowscale=True, alpha=1.25),
    _plain("t2_128_gelu", 300, 256, 128, "T2_128", act=ACT_GELU, outs=PRE, rowscale=True),
    _plain("t2_128_relu", 300, 256, 128, "T2_128", act=ACT_RELU, outs=("out_f32", "out_bf16")),
    _plain("t2_128_gelu_grad", 300, 256, 128, "T2_128", act=ACT_GELU_GRAD, outs=PRE),
    _plain("t2_128_add_f32", 300, 256, 128, "T2_128", aux=AUX_ADD_F32, alpha=0.5),
    _plain("t2_128_add_bf16", 300, 256, 128, "T2_128", aux=AUX_ADD_BF16, outs=BF16),
    _plain("t2_128_mul_bf16", 300, 256, 128, "T2_128", aux=AUX_MUL_BF16, outs=BF16),
    _plain("t2_128_mul_dgelu", 300, 256, 128, "T2_128", aux=AUX_MUL_DGELU, outs=BF16),
    _plain("t2_128_mul_pos", 300, 256, 128, "T2_128", aux=AUX_MUL_POS, outs=BF16, alpha=1.25),
    _plain("t2_128_ragged", 129, 127, 64, "T2_128", outs=("out_f32", "out_bf16"), note="one row / column past a tile"),
    _plain("t2_128_ragged_2", 255, 65, 128, "T2_128", outs=F32),
    # ---- 3-stage ring 64x128 (tall and narrow: the 128x128 grid would not cover the chip)
    _plain("t2_64_ring_none", 2100, 70, 64, "T2_64_RING", outs=("out_f32", "out_bf16")),
    _plain("t2_64_ring_mul_pos", 8512, 192, 1536, "T2_64_RING", aux=AUX_MUL_POS, outs=BF16, bias=False, alpha=1.25),
    _plain("t2_64_ring_ragged", 2049, 129, 192, "T2_64_RING", outs=F32),
    # ---- split-K (accumulate): 8-phase slices through a workspace, 128x128 atomically / through a workspace
    _plain("g8_splitk", 691, 1536, 64 * 260, "G8_SPLITK", bias=False, splitk=4, ws=24 << 20, splitk_out=13, k8_per=20, fold=True),
    _plain("g8_splitk_bump", 700, 1100, 64 * 132, "G8_SPLITK", bias=False, splitk=4, ws=24 << 20, splitk_out=11, k8_per=12,
           fold=True, note="the last slice would hold 2 K-tiles: per grows by 2"),
    _plain("g8_splitk_ws_small", 691, 1536, 64 * 260, "T2_128_SPLITK", bias=False, splitk=4, ws=4 * 691 * 1536,
           splitk_out=4, fold=True, note="the workspace holds the 4 requested slices, not the 13 of the 8-phase plan"),
    _plain("t2_128_splitk_atomic", 192, 320, 64 * 37, "T2_128_SPLITK", bias=False, splitk=8, splitk_out=8),
    _plain("t2_128_splitk_ws", 192, 318, 64 * 37, "T2_128_SPLITK", bias=False, splitk=8, ws=1 << 20, splitk_out=8, fold=True),
    # ---- adapter down-projection (ReLU + dropout in the epilogue): never on the 8-phase kernel
    Route("adapter_down_ring", ADAPTER_DOWN, 8512, 192, 1536, one("T2_64_RING", 8512), drop=True),
    Route("adapter_down_t2_128", ADAPTER_DOWN, 300, 96, 128, one("T2_128", 300), drop=True),
    Route("adapter_down_big_shape", ADAPTER_DOWN, 4100, 2052, 256, one("T2_128", 4100), drop=True,
          note="a big-tile shape: dropout keeps it off the big tiles"),
    # ---- dense + adapter-down: segment output on 8-phase tiles and on narrow tiles
    Route("dense_g8_256", DENSE, 8512, 1536 + 192, 256, one("G8_256", 8512), seg_n=1536, outs=("out_f32", "out_bf16"), drop=True),
    Route("dense_n1_1152", DENSE, 8512, 1152 + 144, 256, one("T2_128", 8512), seg_n=1152, outs=("out_f32", "out_bf16"), drop=True,
          note="N1 % 256 != 0: the wide tiles would cut a wave's column ranges"),
    Route("dense_n1_192", DENSE, 2500, 192 + 24, 128, one("T2_64_RING", 2500), seg_n=192, outs=("out_bf16",), drop=True),
    Route("dense_split", DENSE, 9728, 1536 + 192, 1536, (("T2_64_RING", 9216, 512, False), ("G8_256", 0, 9216, False)),
          seg_n=1536, outs=("out_bf16",), drop=True, note="remainder rows 9216..9727 keep their global dropout keys"),
    Route("dense_split_aux", DENSE, 9728, 1536 + 192, 1536, (("T2_64_RING", 9216, 512, True), ("G8_256", 0, 9216, False)),
          seg_n=1536, outs=("out_bf16",), drop=True, aux_stream=True),
    # ---- adapter tail (up-projection + residual + dropout): never split, never on the 8-phase kernel
    Route("tail_t2_224", TAIL, 8512, 1536, 192, one("T2_224", 8512), drop=True),
    Route("tail_t2_128", TAIL, 1000, 768, 128, one("T2_128", 1000), drop=True, r_norm=True),
]

BY_NAME = {r.name: r for r in ROUTES}
assert len(BY_NAME) == len(ROUTES)

# The (8-phase tile height, epilogue) pairs gemm8_supports admits -- written out, not derived from the plan
GEMM8_PAIRS = {(256, e) for e in ("NONE", "GELU", "GELU_GRAD", "ADD_F32", "ADD_BF16", "MUL_BF16", "MUL_DGELU")} | \
              {(224, "NONE"), (224, "ADD_F32"), (128, "NONE"), (128, "ADD_F32")}


def epilogue_name(r: Route) -> str:
    if r.entry in (ADAPTER_DOWN,):
        return "RELU"
    if r.entry == TAIL:
        return "TAIL"
    if r.act != ACT_NONE:
        return ACT_NAMES[r.act]
    return AUX_NAMES[r.aux]
