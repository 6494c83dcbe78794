"""Every route of the NT GEMM (tests/gemm_routes.py) run through its real entry point on the MI355X and compared with a
float64 reference computed on the GPU from the same bf16 operands.

Two passes per route:
  * exact integers: operands in [-2, 2], integer bias / aux / row scales / prefill / residual, alpha in {1, 0.5, 1.25},
    dropout p = 0.5 (kept values x2).  Every partial sum is then exact in fp32, so fp32 outputs must equal the fp64 reference
    bit for bit and bf16 outputs must equal it rounded to bf16 (RNE, like the kernels' f2bf).  A row, column or K-step in the
    wrong place cannot hide in a tolerance.  (GELU, GELU_GRAD and MUL_DGELU outputs, and GELU_GRAD's saved gelu', are not
    exact: they take the bound below with no accumulation term.)
  * random data: unit normal operands rounded to bf16.  Per element
        |got - ref| <= 2 * K * 2^-24 * (|alpha * rowscale| * |A|.|B|^T)  + the epilogue's own roundings
    (+ 2^-8 |ref| for bf16 outputs: RNE to 8 significand bits).  Why c = 2 is enough: bf16 x bf16 products are exact in fp32, and each of the at most K
    fp32 additions that sum them is off by at most one ulp (2^-23 relative) of a partial sum bounded by |A|.|B|^T -- even
    with truncating instead of rounding additions.  A missing or duplicated 64-deep K-tile moves an element by about
    sqrt(64) x the operand scale, far outside it.  The epilogue terms are written out in `bound`.
Outputs live in buffers with a tile of extra rows and ldc > N, filled with a NaN sentinel that must survive bit for bit
outside [0, M) x [0, N).  Failures name the launches fbl_gemm_plan_launches reports for the device's CU count, with the
number of bad elements in each launch's row range.
"""
import math

import pytest
import torch

from tests.dropout_replay import row_mask
from tests.gemm_routes import (ACT_GELU, ACT_GELU_GRAD, ACT_NONE, ACT_RELU, ADAPTER_DOWN, AUX_ADD_BF16, AUX_ADD_F32,
                               AUX_MUL_BF16, AUX_MUL_DGELU, AUX_MUL_POS, AUX_NONE, DENSE, PLAIN, ROUTES, TAIL, Route)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
SENT = {F32: 0x7FC0DEAD, BF16: 0x7FA5}  # NaN bit patterns
IVIEW = {F32: torch.int32, BF16: torch.int16}
GUARD_ROWS = 256


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


@pytest.fixture(scope="module")
def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def aux_stream():
    return torch.cuda.Stream()


# ------------------------------------------------------------------------------------------------ data and buffers
class Gen:
    def __init__(self, seed, exact):
        self.g = torch.Generator(device=DEV).manual_seed(seed)
        self.exact = exact

    def val(self, *shape, lo=-2, hi=2, scale=1.0):
        """integers in [lo, hi] (exact pass) or unit normals * scale rounded to bf16 (random pass), as fp32"""
        if self.exact:
            return torch.randint(lo, hi + 1, shape, generator=self.g, device=DEV).float()
        return (torch.randn(*shape, generator=self.g, device=DEV) * scale).to(BF16).float()


def operand(vals, ld):
    """bf16 [rows, cols] view with row stride ld; the padding columns hold NaN (a read past K would poison the result)"""
    rows, cols = vals.shape
    full = torch.empty(rows, ld, dtype=BF16, device=DEV)
    full.view(torch.int16).fill_(SENT[BF16])
    full[:, :cols] = vals.to(BF16)
    return full[:, :cols]


def guarded(rows, cols, ld, dtype, fill=None):
    """output buffer [rows + GUARD_ROWS, ld] of sentinels; returns (full, view [rows, cols]) -- view prefilled with `fill`"""
    full = torch.empty(rows + GUARD_ROWS, ld, dtype=dtype, device=DEV)
    full.view(IVIEW[dtype]).fill_(SENT[dtype])
    view = full[:rows, :cols]
    if fill is not None:
        view.copy_(fill)
    return full, view


def guard_intact(full, rows, cols):
    bits = full.view(IVIEW[full.dtype])
    s = SENT[full.dtype]
    return bool((bits[:, cols:] == s).all()) and bool((bits[rows:, :cols] == s).all())


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def dgelu64(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------ one call of a route
P_DROP = {True: 0.5, False: 0.25}  # exact pass: kept values x2 (exact)
SEED = 0x5EED1234


def make_inputs(r: Route, exact: bool, seed: int):
    g = Gen(seed, exact)
    M, N, K = r.M, r.N, r.K
    d = dict(A=g.val(M, K), B=g.val(N, K))
    d["bias"] = g.val(N, lo=-8, hi=8) if r.bias else None
    d["rowscale"] = g.val(M, lo=0, hi=2).abs() if r.rowscale else None
    if r.entry == PLAIN and r.aux != AUX_NONE:
        d["aux"] = g.val(M, N, lo=-4, hi=4)
    if r.entry == PLAIN and r.splitk > 1:
        d["prefill"] = g.val(M, N, lo=-50, hi=50, scale=10.0)
    if r.entry == TAIL:
        d["x"] = g.val(M, N, lo=-16, hi=16)
        d["r"] = g.val(M, N, lo=-16, hi=16, scale=2.0) if exact else torch.randn(M, N, generator=g.g, device=DEV)
        if r.r_norm and not exact:
            d["stats"] = torch.stack([torch.randn(M, generator=g.g, device=DEV) * 0.1,
                                      torch.rand(M, generator=g.g, device=DEV) + 0.5], 1).contiguous()
            d["gamma"] = 1 + 0.1 * torch.randn(N, generator=g.g, device=DEV)
            d["beta"] = 0.1 * torch.randn(N, generator=g.g, device=DEV)
            d["rowmask"] = (torch.arange(M, device=DEV) % 7 != 0).to(torch.int32)
    return d


def run(L, r: Route, d, exact: bool):
    """calls the entry point; returns {output name: (full buffer, rows, cols)}"""
    M, N, K = r.M, r.N, r.K
    A, B = operand(d["A"], r.lda), operand(d["B"], r.ldb)
    p = P_DROP[exact] if r.drop else 0.0
    outs = {}
    if r.entry == PLAIN:
        kw = {}
        for name, dt in (("out_f32", F32), ("out_bf16", BF16), ("out_pre", BF16)):
            if name in r.outs:
                full, view = guarded(M, N, r.ldc, dt, d.get("prefill") if name == "out_f32" else None)
                outs[name] = (full, M, N)
                kw[name] = view
        if r.aux != AUX_NONE:
            dt = F32 if r.aux == AUX_ADD_F32 else BF16
            kw["aux"] = guarded(M, N, r.ld_aux, dt, d["aux"])[1]
            kw["aux_kind"] = r.aux
        ws = torch.empty(r.ws, dtype=F32, device=DEV) if r.ws is not None else None
        L.gemm(A, B, bias=d["bias"], rowscale=d["rowscale"], alpha=r.alpha, act=r.act, splitk=r.splitk, ws=ws, N=N, **kw)
    elif r.entry == ADAPTER_DOWN:
        full, z = guarded(M, N, r.ldc, BF16)
        outs["z"] = (full, M, N)
        L.adapter_down_fwd(A, B, d["bias"], z, p_drop=p, seed=SEED)
    elif r.entry == DENSE:
        N1, Aw = r.seg_n, N - r.seg_n
        kw = {}
        for name, dt, key in (("out_f32", F32, "y_f32"), ("out_bf16", BF16, "y_bf16")):
            if name in r.outs:
                full, view = guarded(M, N1, r.ldc, dt)
                outs[key] = (full, M, N1)
                kw[key] = view
        full, z = guarded(M, Aw, r.ld_aux, BF16)
        outs["z"] = (full, M, Aw)
        L.dense_adapter_down_fwd(A, B, d["bias"], N1, z, p_drop=p, seed=SEED, **kw)
    else:
        full, t = guarded(M, N, r.ldc, F32)
        outs["t"] = (full, M, N)
        x = guarded(M, N, r.ld_aux, BF16, d["x"])[1]
        rt = guarded(M, N, r.ldc, F32, d["r"])[1]  # (the residual shares the output's row stride, as the query assumes)
        if "stats" in d:
            L.adapter_up_resid_fwd(A, B, d["bias"], x, t, p_drop=p, seed=SEED,
                                   r_norm=(rt, d["stats"], d["gamma"], d["beta"], d["rowmask"]))
        else:
            L.adapter_up_resid_fwd(A, B, d["bias"], x, t, p_drop=p, seed=SEED, r_plain=rt)
    torch.cuda.synchronize()
    return outs


def reference(r: Route, d, exact: bool):
    """{output name: (ref fp64, bound fp64 or None (bit-exact), dtype)}"""
    M, N, K = r.M, r.N, r.K
    A, B = d["A"].double(), d["B"].double()
    acc = A @ B.t()
    absacc = 0.0 if exact else (A.abs() @ B.abs().t())
    kacc = 2.0 * K * U  # accumulation bound factor (see the module docstring)
    alpha = r.alpha
    rs = d["rowscale"].double()[:, None] if d["rowscale"] is not None else 1.0
    bias = d["bias"].double()[None] if d["bias"] is not None else 0.0
    v = (alpha * acc + bias) * rs
    rsa = rs.abs() if torch.is_tensor(rs) else 1.0
    ba = bias.abs() if torch.is_tensor(bias) else 0.0
    # accumulation, then the (at most three) roundings of alpha * acc + bias and * rowscale
    vb = (kacc * abs(alpha) * absacc + 4 * U * ((alpha * acc).abs() + ba)) * rsa
    fn = 2.0 ** -20  # erf / exp approximations of the GELU epilogues (|abs err of erf| <= 1.5e-7 < 2^-22), generously
    res = {}

    def add(name, ref, bound, dt, exact_ok):
        if dt == BF16:
            # RNE to 8 significand bits: off by at most half an ulp = 2^-8 of the value's binade, i.e. <= 2^-8 |x|
            bound = None if (exact and exact_ok) else (bound * 1.01 + 2.0 ** -8 * ref.abs() * 1.01)
        else:
            bound = None if (exact and exact_ok) else bound
        res[name] = (ref, bound, dt)

    if r.entry == PLAIN:
        if r.splitk > 1:
            add("out_f32", d["prefill"].double() + acc, vb + 2 * U * (d["prefill"].double().abs() + acc.abs()), F32, True)
            return res
        out, ob, pre, pb, exact_out, exact_pre = v, vb, v, vb, True, True
        if r.act == ACT_GELU:
            out, ob, exact_out = gelu64(v), 1.13 * vb + fn * (v.abs() + 1), False
        elif r.act == ACT_RELU:
            out = torch.relu(v)
        elif r.act == ACT_GELU_GRAD:
            out, ob, exact_out = gelu64(v), 1.13 * vb + fn * (v.abs() + 1), False
            pre, pb, exact_pre = dgelu64(v), vb + fn * (v.abs() + 1), False
        if r.aux != AUX_NONE:
            x = d["aux"].double()
            if r.aux in (AUX_ADD_F32, AUX_ADD_BF16):
                out, ob = out + x, ob + 2 * U * (out + x).abs()
            elif r.aux == AUX_MUL_DGELU:
                dg = dgelu64(x)
                out, ob, exact_out = out * dg, ob * dg.abs() + out.abs() * fn * (1 + x.abs()) + 2 * U * (out * dg).abs(), False
            elif r.aux == AUX_MUL_POS:
                out, ob = torch.where(x > 0, out, torch.zeros_like(out)), torch.where(x > 0, ob, torch.zeros_like(ob))
            elif r.aux == AUX_MUL_BF16:
                out, ob = out * x, ob * x.abs() + 2 * U * (out * x).abs()
        if "out_f32" in r.outs:
            add("out_f32", out, ob, F32, exact_out)
        if "out_bf16" in r.outs:
            add("out_bf16", out, ob, BF16, exact_out)
        if "out_pre" in r.outs:
            add("out_pre", pre, pb, BF16, exact_pre)
        return res
    p = P_DROP[exact] if r.drop else 0.0
    if r.entry == ADAPTER_DOWN:
        mask = row_mask(SEED, (M, N), p, ld=r.ldc).to(DEV).double() if p else 1.0
        z = torch.relu(v) * mask
        add("z", z, vb * (mask if p else 1.0) + 2 * U * z.abs(), BF16, True)
        return res
    if r.entry == DENSE:
        N1 = r.seg_n
        if "out_f32" in r.outs:
            add("y_f32", v[:, :N1], vb[:, :N1], F32, True)
        if "out_bf16" in r.outs:
            add("y_bf16", v[:, :N1], vb[:, :N1], BF16, True)
        mask = row_mask(SEED, (M, N - N1), p, ld=r.ld_aux).to(DEV).double() if p else 1.0
        z = torch.relu(v[:, N1:]) * mask
        add("z", z, vb[:, N1:] * (mask if p else 1.0) + 2 * U * z.abs(), BF16, True)
        return res
    # adapter tail: t = dropout(alpha*acc + bias + x) + residual; dropout keys (seed, m*H + n)
    x = d["x"].double()
    y = v + x
    yb = vb + 2 * U * y.abs()
    mask = row_mask(SEED, (M, N), p, ld=N).to(DEV).double() if p else 1.0
    if "stats" in d:
        st = d["stats"].double()
        c = d["r"].double() - st[:, :1]
        resid = (c * st[:, 1:] * d["gamma"].double()[None] + d["beta"].double()[None]) * d["rowmask"].double()[:, None]
        rb = 8 * U * (c.abs() * st[:, 1:].abs() * d["gamma"].double().abs()[None] + d["beta"].double().abs()[None])
    else:
        resid, rb = d["r"].double(), 0.0
    t = y * mask + resid
    add("t", t, yb * (mask if p else 1.0) + rb + 2 * U * t.abs(), F32, True)
    return res


def describe(plan, bad):
    """bad elements per launch row range"""
    rows = bad.any(1)
    parts = []
    for k, row0, n, on_aux in plan["launches"]:
        parts.append(f"{k}[{row0}:{row0 + n}]{'(aux)' if on_aux else ''}: {int(bad[row0:row0 + n].sum())} bad")
    return "; ".join(parts) + f"; first bad row {int(rows.nonzero()[0])}" if rows.any() else "; ".join(parts)


def check(r: Route, plan, outs, refs, tag):
    for name, (ref, bound, dt) in refs.items():
        full, rows, cols = outs[name]
        got = full[:rows, :cols]
        assert guard_intact(full, rows, cols), f"{r.name} {tag} {name}: wrote outside [0,{rows})x[0,{cols}); launches {plan['launches']}"
        if bound is None:
            want = ref.to(dt)
            bad = got.view(IVIEW[dt]) != want.view(IVIEW[dt])
            # (+0 / -0 are the same value)
            bad &= ~((got == 0) & (want == 0))
        else:
            g64 = got.double()
            bad = ~((g64 - ref).abs() <= bound)
        if bool(bad.any()):
            i = bad.nonzero()[0].tolist()
            detail = (f"got {got[i[0], i[1]].item()!r} ref {ref[i[0], i[1]].item()!r}"
                      + (f" bound {bound[i[0], i[1]].item():.3e}" if bound is not None and torch.is_tensor(bound) else ""))
            pytest.fail(f"{r.name} {tag} {name}: {int(bad.sum())} bad elements, first at {tuple(i)}: {detail}; "
                        f"{describe(plan, bad)}")


def bits(outs):
    return {k: full.view(IVIEW[full.dtype]).clone() for k, (full, _, _) in outs.items()}


# ------------------------------------------------------------------------------------------------ the route tests
@pytest.mark.parametrize("route", ROUTES, ids=[r.name for r in ROUTES])
def test_route_against_fp64(L, n_cu, aux_stream, route):
    r = route
    L.set_aux_stream(aux_stream if r.aux_stream else None)
    try:
        code, plan = r.query(L, n_cu)
        assert code == 0, (r.name, code)
        if n_cu == 256:
            assert tuple(tuple(l) for l in plan["launches"]) == r.expect, (r.name, plan)
        # exact integers
        d = make_inputs(r, True, 11)
        outs = run(L, r, d, True)
        check(r, plan, outs, reference(r, d, True), "exact")
        if len(plan["launches"]) == 2:  # the two-launch plans give the same bits with and without the aux stream
            L.set_aux_stream(None if r.aux_stream else aux_stream)
            outs2 = run(L, r, d, True)
            L.set_aux_stream(aux_stream if r.aux_stream else None)
            for k, b in bits(outs).items():
                assert torch.equal(b, bits(outs2)[k]), f"{r.name} {k}: aux stream on / off differ; launches {plan['launches']}"
        del outs, d
        # random data, twice: within the bound, and bit-reproducible unless the route adds atomically
        d = make_inputs(r, False, 12)
        outs = run(L, r, d, False)
        check(r, plan, outs, reference(r, d, False), "random")
        atomic = r.splitk > 1 and r.ws is None
        if not atomic:
            b1 = bits(outs)
            del outs
            outs = run(L, r, d, False)
            for k, b in bits(outs).items():
                assert torch.equal(b, b1[k]), f"{r.name} {k}: two calls differ; launches {plan['launches']}"
    finally:
        L.set_aux_stream(None)


def test_dropout_pattern_of_the_split_remainder_rows(L, n_cu):
    """The M = 9728 dense + adapter-down split: the remainder launch (rows 9216..9727, 64x128 tiles) keys its dropout with the
    global row (drop_row0): its kept / dropped pattern is the host rebuild's, element for element."""
    r = next(x for x in ROUTES if x.name == "dense_split")
    code, plan = r.query(L, n_cu)
    assert code == 0
    d = make_inputs(r, True, 21)
    d["A"] = d["A"].abs() + 1  # (all-positive operands: relu(v) > 0 everywhere, so every dropped element shows)
    d["B"] = d["B"].abs() + 1
    outs = run(L, r, d, True)
    z = outs["z"][0][:r.M, :r.N - r.seg_n]
    keep = row_mask(SEED, (r.M, r.N - r.seg_n), 0.5, ld=r.ld_aux).to(DEV) > 0
    got = z.float() != 0
    for k, row0, n, _ in plan["launches"]:
        diff = int((got[row0:row0 + n] != keep[row0:row0 + n]).sum())
        assert diff == 0, f"{k} rows [{row0}, {row0 + n}): {diff} elements kept / dropped against the host rebuild"


# ------------------------------------------------------------------------------------------------ the other GEMM-shaped kernels
@pytest.mark.parametrize("K,M,N", [(8512, 1536, 192), (333, 192, 1536), (64, 16, 128), (1000, 128, 16), (77, 72, 200)])
def test_gemm_tn_acc_exact(L, K, M, N):
    """fbl_gemm_bf16_tn_acc on integer data (its four test shapes and a ragged K): bit-equal to fp64, accumulated into an
    integer prefill; nothing outside [0, M) x [0, N) written."""
    g = Gen(31, True)
    Mp, Np = (M + 63) // 64 * 64, (N + 63) // 64 * 64
    A = torch.zeros(K, Mp, dtype=BF16, device=DEV); A[:, :M] = g.val(K, M).to(BF16)
    B = torch.zeros(K, Np, dtype=BF16, device=DEV); B[:, :N] = g.val(K, N).to(BF16)
    pre = g.val(M, N, lo=-50, hi=50)
    full, out = guarded(M, N, N + 8, F32, pre)
    ws = torch.empty(16 << 20, dtype=F32, device=DEV)
    L.gemm_tn_acc(A, B, out, ws, M=M, N=N, K=K, splitk=8)
    ref = pre.double() + A[:, :M].double().t() @ B[:, :N].double()
    assert guard_intact(full, M, N)
    assert torch.equal(out.double(), ref), (out.double() - ref).abs().max().item()


@pytest.mark.parametrize("N,H,A,nad", [(8512, 1536, 192, 2), (333, 128, 16, 3)])
def test_adapter_bwd_dw_exact(L, N, H, A, nad):
    """fbl_adapter_bwd_dw on integer data: dWu += sum dy^T z, dWd += sum dz^T x, dbd += sum colsum(dz) bit-equal to fp64
    (the first adapter has two segments)."""
    g = Gen(41, True)
    Ap = (A + 63) // 64 * 64

    def seg():
        dy = g.val(N, H).to(BF16)
        z = torch.zeros(N, Ap, dtype=BF16, device=DEV); z[:, :A] = g.val(N, A, lo=0, hi=3).to(BF16)
        dz = torch.zeros(N, Ap, dtype=BF16, device=DEV); dz[:, :A] = g.val(N, A).to(BF16)
        x = g.val(N, H).to(BF16)
        return dy, z, dz, x

    segs = [[seg() for _ in range(2 if o == 0 else 1)] for o in range(nad)]
    grp = [(segs[o], torch.full((H, A), 3.0, device=DEV), torch.full((A, H), -5.0, device=DEV), torch.full((A,), 7.0, device=DEV))
           for o in range(nad)]
    L.adapter_bwd_dw(grp, A=A)
    for sg, dWu, dWd, dbd in grp:
        assert torch.equal(dWu.double(), 3.0 + sum(dy.double().t() @ z[:, :A].double() for dy, z, dz, x in sg))
        assert torch.equal(dWd.double(), -5.0 + sum(dz[:, :A].double().t() @ x.double() for dy, z, dz, x in sg))
        assert torch.equal(dbd.double(), 7.0 + sum(dz[:, :A].double().sum(0) for dy, z, dz, x in sg))
