"""CPU: the NT GEMM's launch plan (fbl_gemm_plan_launches: the entry points' own validation and planner, no HIP call).

The route table (tests/gemm_routes.py) pins the launches of every kernel configuration and of both outcomes of each
planner decision at 256 CUs; a deterministic sweep checks the plan's invariants over shapes at the tile boundaries, every
option and several CU counts."""
import random

import pytest

from tests.gemm_routes import (ADAPTER_DOWN, DENSE, GEMM8_PAIRS, KERNELS, PLAIN, ROUTES, TAIL, epilogue_name)

ERR_SHAPE, ERR_ALIGN, ERR_ARG = -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib
    from frozenbilm_amd.build import build_lib

    lib.load(build_lib(verbose=False))
    return lib


@pytest.mark.parametrize("route", ROUTES, ids=[r.name for r in ROUTES])
def test_route_table_at_256_cus(L, route):
    code, plan = route.query(L, 256)
    assert code == 0, (route.name, code)
    got = tuple(tuple(l) for l in plan["launches"])
    assert got == route.expect, (route.name, got)
    assert (plan["splitk"], plan["k8_per"], plan["fold"]) == (route.splitk_out, route.k8_per, route.fold), (route.name, plan)


def test_route_table_covers_every_kernel_and_gemm8_epilogue(L):
    kernels = {l[0] for r in ROUTES for l in r.expect}
    assert kernels == set(KERNELS), set(KERNELS) - kernels
    heights = {"G8_256": 256, "G8_224": 224, "G8_128": 128}
    pairs = {(heights[l[0]], epilogue_name(r)) for r in ROUTES for l in r.expect if l[0] in heights}
    assert pairs == GEMM8_PAIRS, GEMM8_PAIRS ^ pairs
    # the 2-stage kernels: every epilogue of launch_one on at least one tile height, NONE on all four heights
    t2 = {"T2_256", "T2_224", "T2_128", "T2_64_RING"}
    epis = {epilogue_name(r) for r in ROUTES for l in r.expect if l[0] in t2}
    assert epis >= {"NONE", "GELU", "RELU", "GELU_GRAD", "ADD_F32", "ADD_BF16", "MUL_DGELU", "MUL_POS", "MUL_BF16", "TAIL"}, epis
    assert t2 <= {l[0] for r in ROUTES for l in r.expect if epilogue_name(r) == "NONE"}
    # the G8_128 entry really is what the planner gives the N = 1536 dX GEMM at a packed-row count
    code, plan = L.gemm_plan_launches(PLAIN, 5322, 1536, 6144, opts=("out_bf16",))
    assert code == 0 and plan["launches"] == [("G8_128", 0, 5322, False)]


def test_route_table_decisions_have_both_outcomes():
    names = {r.name for r in ROUTES}
    for pair in [("g8_224_none", "g8_256_none"),                     # r224 / 256
                 ("single_launch_qkv", "split_ring_rem"),            # the single_launch window
                 ("split_ring_rem", "split_t2_128_rem"),             # remainder on 64x128 / 128x128 tiles
                 ("split_rounds_t2_256", "split_rounds_t2_128"),     # whole rounds falling back
                 ("g8_128_none", "g8_128_rejected"),                 # the G8_128 cost model
                 ("g8_splitk", "g8_splitk_bump", "g8_splitk_ws_small"),
                 ("t2_128_splitk_atomic", "t2_128_splitk_ws"),
                 ("dense_g8_256", "dense_n1_1152", "dense_split"),
                 ("tail_t2_224", "tail_t2_128"),
                 ("t2_256_nk2", "t2_256_nk3", "t2_224_odd")]:
        assert set(pair) <= names, pair


# What the comments of the GEMM tests in test_gpu_kernels.py say each shape runs on (256 CUs): kept true here
EXISTING_TEST_ROUTES = {
    # test_gemm_plain_bias (out_f32 + out_bf16 + bias)
    (PLAIN, 4100, 3500, 256): ["G8_256"], (PLAIN, 4100, 3584, 1536): ["G8_256"],
    (PLAIN, 8512, 6144, 384): ["T2_64_RING", "G8_256"], (PLAIN, 8512, 6144, 1536): ["T2_64_RING", "G8_256"],
    (PLAIN, 8512, 1536, 384): ["G8_224"], (PLAIN, 4100, 2052, 256): ["G8_224"],
    (PLAIN, 4100, 2052, 128): ["T2_224"], (PLAIN, 8512, 1536, 192): ["T2_224"], (PLAIN, 4100, 3584, 128): ["T2_256"],
    (PLAIN, 8512, 192, 1536): ["T2_64_RING"], (PLAIN, 2100, 70, 64): ["T2_64_RING"], (PLAIN, 691, 16500, 256): ["G8_256"],
    (PLAIN, 4100, 4608, 256): ["T2_64_RING", "G8_256"], (PLAIN, 4100, 4500, 192): ["T2_64_RING", "T2_256"],
    (PLAIN, 2500, 8192, 128): ["T2_128", "T2_256"],
    # test_dense_adapter_down_merged (M, N1 + A, K, N1)
    (DENSE, 300, 144, 128, 128): ["T2_128"], (DENSE, 4100, 1728, 256, 1536): ["T2_128"],
    (DENSE, 8512, 1728, 1536, 1536): ["G8_256"],
    (DENSE, 2500, 216, 128, 192): ["T2_64_RING"], (DENSE, 4100, 1296, 256, 1152): ["T2_128"],
    (DENSE, 8512, 1296, 256, 1152): ["T2_128"],
}


@pytest.mark.parametrize("key", list(EXISTING_TEST_ROUTES), ids=[str(k) for k in EXISTING_TEST_ROUTES])
def test_comments_of_the_kernel_tests_match_the_plan(L, key):
    entry, M, N, K = key[:4]
    if entry == DENSE:
        code, plan = L.gemm_plan_launches(DENSE, M, N, K, seg_n=key[4], ldc=key[4], ld_aux=N - key[4],
                                          opts=("out_f32", "out_bf16", "bias"))
    else:
        code, plan = L.gemm_plan_launches(PLAIN, M, N, K, ldc=(N + 7) // 8 * 8, opts=("out_f32", "out_bf16", "bias"))
    assert code == 0 and [l[0] for l in plan["launches"]] == EXISTING_TEST_ROUTES[key], (key, plan)


def test_query_returns_the_entry_points_error_codes(L):
    q = L.gemm_plan_launches
    assert q(PLAIN, 100, 100, 100, opts=("out_f32",))[0] == ERR_SHAPE       # K % 64
    assert q(PLAIN, 100, 100, 128, lda=132, opts=("out_f32",))[0] == ERR_ALIGN
    assert q(PLAIN, 100, 100, 128, opts=())[0] == ERR_ARG                 # no output
    assert q(PLAIN, 100, 100, 128, opts=("out_f32", "bias", "ws"), splitk=2, ws_floats=1 << 20)[0] == ERR_ARG
    assert q(PLAIN, 100, 100, 128, opts=("out_bf16",), splitk=2)[0] == ERR_ARG
    assert q(PLAIN, 100, 100, 128, aux_kind=6, opts=("out_f32", "aux"))[0] == ERR_ARG  # the tail has its own entry point
    assert q(DENSE, 100, 100 + 64, 128, seg_n=100, opts=("out_f32",))[0] == ERR_ARG  # N1 % 64
    assert q(TAIL, 100, 130, 128, ld_aux=136, ldc=132)[0] == ERR_ARG               # H % 4
    assert q(TAIL, 100, 128, 128, ld_aux=132, ldc=128)[0] == ERR_ALIGN            # ldx % 8
    assert q(PLAIN, 100, 100, 128, opts=("out_f32",), n_cu=0)[0] == ERR_ARG
    code, plan = q(PLAIN, 0, 100, 128, opts=("out_f32",))
    assert code == 0 and plan["launches"] == []                                   # nothing to do


def _gemm8_eligible(rows, lda, N, ldb, K):
    nk = K // 64
    return K % 64 == 0 and nk % 2 == 0 and nk >= 4 and rows * lda * 2 < 1 << 32 and N * ldb * 2 < 1 << 32


MS = [1, 63, 64, 65, 127, 128, 129, 223, 224, 225, 255, 256, 257, 511, 512, 513, 691, 1023, 1024, 1025, 1500, 2047, 2048,
      2049, 4100, 5322, 8191, 8192, 8193, 8512, 9024, 9728]
NS = [4, 64, 65, 127, 128, 129, 192, 255, 256, 257, 1023, 1024, 1025, 1296, 1536, 1728, 2052, 3584, 4608, 6144, 8192, 8448,
      16384, 16500, 32768]
KS = [64, 128, 192, 256, 320, 384, 1536, 6144, 64 * 129, 64 * 130, 64 * 132, 64 * 260]


def _sweep(n):
    rng = random.Random(1234)
    for _ in range(n):
        entry = rng.choice([PLAIN] * 5 + [ADAPTER_DOWN, DENSE, DENSE, TAIL])
        M, K = rng.choice(MS), rng.choice(KS)
        c = dict(entry=entry, M=M, K=K, n_cu=rng.choice([256, 128, 80, 32]), opts=set(), batch=1, splitk=1, ws_floats=0,
                 seg_n=0, act=0, aux_kind=0)
        c["lda"] = K + rng.choice([0, 0, 8, 64])
        if entry == PLAIN:
            N = rng.choice(NS)
            c["opts"] |= set(rng.choice([("out_f32",), ("out_bf16",), ("out_f32", "out_bf16"), ("out_bf16", "out_pre")]))
            c["act"], c["aux_kind"] = rng.choice([(0, 0), (0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5)])
            if c["aux_kind"]:
                c["opts"].add("aux")
            c["batch"] = rng.choice([1, 1, 1, 2])
            if rng.random() < 0.35:
                c["splitk"] = rng.choice([2, 4, 8])
                c["act"], c["aux_kind"] = 0, 0
                c["opts"] = {"out_f32"}
        elif entry == ADAPTER_DOWN:
            N = rng.choice([16, 96, 192, 256, 2052])
        elif entry == DENSE:
            N1 = rng.choice([64, 192, 768, 1152, 1536, 3072])
            N = N1 + rng.choice([16, 96, 144, 192, 256])
            c["seg_n"] = N1
            c["opts"] |= set(rng.choice([("out_f32",), ("out_bf16",), ("out_f32", "out_bf16")]))
        else:
            N = rng.choice([128, 768, 1536])
            c["ld_aux"] = N + 8
            if rng.random() < 0.5:
                c["opts"].add("r_norm")
        c["N"] = N
        c["ldc"] = N + rng.choice([0, 4, 8]) if entry != DENSE else N - c["seg_n"] + 8
        if entry == DENSE:
            c["ld_aux"] = N - c["seg_n"] + 8
        if rng.random() < 0.5:
            c["opts"].add("bias")
        if entry == PLAIN and rng.random() < 0.2:
            c["opts"].add("rowscale")
        if entry != PLAIN and rng.random() < 0.6:
            c["opts"].add("dropout")
        if rng.random() < 0.4:
            c["opts"].add("ws")
            c["ws_floats"] = rng.choice([1 << 10, 1 << 20, 24 << 20, 1 << 28])
        if rng.random() < 0.5:
            c["opts"].add("aux_stream")
        yield c


def test_plan_invariants_over_a_sweep(L):
    n_ok = 0
    seen = set()
    for c in _sweep(4000):
        opts = tuple(sorted(c["opts"]))
        code, plan = L.gemm_plan_launches(c["entry"], c["M"], c["N"], c["K"], lda=c["lda"], ldb=c["lda"], ldc=c["ldc"],
                                          ld_aux=c.get("ld_aux", 0), seg_n=c["seg_n"], act=c["act"], aux_kind=c["aux_kind"],
                                          opts=opts, batch=c["batch"], splitk=c["splitk"], ws_floats=c["ws_floats"],
                                          n_cu=c["n_cu"])
        if code:
            continue
        n_ok += 1
        ls = plan["launches"]
        M, N, K = c["M"], c["N"], c["K"]
        nk = K // 64
        seen |= {l[0] for l in ls}
        # the launches partition [0, M), none empty
        spans = sorted((l[1], l[2]) for l in ls)
        assert all(rows > 0 for _, rows in spans), (c, ls)
        assert spans[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:])), (c, ls)
        assert spans[-1][0] + spans[-1][1] == M, (c, ls)
        # at most one launch on the aux stream, and only when one is given
        n_aux = sum(l[3] for l in ls)
        assert n_aux <= 1 and (n_aux == 0 or "aux_stream" in c["opts"]), (c, ls)
        accumulate = c["splitk"] > 1
        if c["entry"] == TAIL or "ws" in c["opts"] or c["batch"] > 1 or accumulate:
            assert len(ls) == 1, (c, ls)
        if len(ls) == 2:  # a split: the remainder (2-stage) first, then the whole rounds from row 0
            assert ls[1][1] == 0 and ls[0][0] in ("T2_64_RING", "T2_128"), (c, ls)
        for k, row0, rows, _ in ls:
            if k in ("G8_256", "G8_224", "G8_128"):
                assert _gemm8_eligible(rows, c["lda"], N, c["lda"], K), (c, ls)
                assert not accumulate and not ("dropout" in c["opts"] and c["seg_n"] <= 0), (c, ls)
            if k == "G8_SPLITK":
                assert nk % 2 == 0 and nk >= 128 and M * c["lda"] * 2 < 1 << 32 and N * c["lda"] * 2 < 1 << 32, (c, ls)
                s8, per = plan["splitk"], plan["k8_per"]
                assert s8 >= 2 and per % 2 == 0 and per >= 8 and (s8 - 1) * per < nk <= s8 * per, (c, plan)
                assert nk - (s8 - 1) * per >= 4 and s8 * M * ((N + 3) & ~3) <= c["ws_floats"], (c, plan)
            if k in ("G8_SPLITK", "T2_128_SPLITK"):
                assert accumulate, (c, ls)
        # the workspace is folded exactly when the call accumulates through a workspace that is large enough
        if accumulate:
            per = -(-nk // c["splitk"])
            sk = -(-nk // per)
            fits = "ws" in c["opts"] and c["batch"] * sk * M * ((N + 3) & ~3) <= c["ws_floats"]
        else:
            fits = False
        assert plan["fold"] == fits, (c, plan)
        # fbl_gemm_plan (plain problem, lda = K, 256 CUs) agrees with the query's big8
        if c["entry"] == PLAIN and c["lda"] == K:
            assert (L.gemm_plan(M, N, K, c["batch"], c["splitk"]) == 8) == plan["big8"], (c, plan)
    assert n_ok > 2500, n_ok
    assert seen == set(KERNELS), set(KERNELS) - seen
