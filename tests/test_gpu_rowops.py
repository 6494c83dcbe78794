"""Every case of the row-op table (tests/rowop_cases.py) run through its C-ABI entry point on the MI355X and compared with a
float64 reference of the same operation (tests/gpu_refs.py), computed on the GPU from the very input bits the kernel gets.
Dropout is never "checked by rate": the keep masks are rebuilt on the host (tests/dropout_replay.row_mask, key m*H + n or the
flat index) and applied inside the reference.

Three kinds of assertion (u = 2^-24):

(a) Exact.  Small-integer inputs make every partial sum exact in fp32 in any order: colsum (fp32 and bf16 input), sumsq (integers
    in [-4, 4], 16 n < 2^24), dbeta with integer dout and a 0/1 row mask, scatter_rows_f32 and dropout_f32 / dropout_bf16 (one fp32
    operation per element: must equal torch's fp32 result), gather_rows_bf16, cast_f32_to_bf16 (torch's RNE, ties and denormals
    included), out_t of ln_fwd without dropout and r_norm (one fp32 addition), the zero pattern of every dropout output, and the
    exact zeros of cross entropy (ignored rows, columns [V, Vp), row_lse of an ignored row).

(b) Derived bounds for plain reductions, per output element, n terms:  |got - ref| <= 2 n u sum|term_i|  (each of at most n fp32
    additions is off by at most one ulp = 2u of a partial sum that sum|term_i| bounds), + 2u |result| for the final "+=" into the
    accumulator, + 2^-8 |ref| for a bf16 output.  sumsq, colsum, the loss sum of ce_fwd, dgamma / dbeta / dysum.  The reductions
    are judged on their own: the fp64 sum takes the kernel's own row_lse / out_dt / (t, stats) as terms.  Where a term is itself
    computed in fp32 before it is summed its roundings are added: dgamma's term dout * (t - mean) * rstd takes three, so
    + 4u sum |dout| rstd (|t| + |mean|); dysum's term dt * 1/(1-p) takes one, so + 2u sum|term|; the loss term lse - logit one.

(c) Measured bounds for what has transcendental or ill-conditioned steps.  Each has a fixed FORM that carries the conditioning
    and one dimensionless constant C.  The constant is never taken from the HIP kernel: the yardstick is a plain fp32 torch
    evaluation of the same formula on the same inputs (torch.native_layer_norm and autograd through it, torch.logsumexp,
    F.cross_entropy, F.gelu, torch.optim.Adam + clip_grad_norm_), its error against the fp64 reference is expressed in the
    form, and C = 4 x the largest yardstick value over all cases of the family, rounded up to a power of two.  Every run
    recomputes the yardstick and asserts it within C / 4, then asserts the kernel within C.

    quantity        form (per element)                                                       yardstick max   C     kernel max
    ln_fwd t        u * ax                     ax = sum of |addends| of t                     3.98            16    3.17
    ln_fwd mean     u * max_row(ax)                                                           3.33            16    2.66
    ln_fwd rstd     u * rstd * (1 + rstd * max_row(ax))   (relative, with the row's condition)  0.61            4     0.55
    ln_fwd out      u * (|gamma| rstd (ax + mean_row(ax)) + |out|) * rowmask (+ 2^-8 |out|)   2.30            16    2.14
    ln_materialize  u * ((|t| + |mean|) rstd |gamma| + |beta| + |pos| + |out|)                1.79            8     1.68
    ln_bwd dt, dy   u * rstd * (|g| + mean|g| + |xhat| mean|g xhat|) [* keep] (+ 2^-8 |dy|)   3.35            16    2.99
    row_lse         u * max(1, |lse|)                                                         1.39            8     2.41
    dlogits         u * (p + onehot) * (max(1, |x - lse|) + |lse|) * scale + 2^-8 |ref| + 2^-126  1.25         8     0.00
    gelu            u * |v|    (v = dropout(c): the input scale; gelu(v) <= |v|)              2.80            16    4.91
    gelu'           u * |dy| * keep * max(|gelu'(v)|, 1)  (+ 2^-8 |ref| bf16)                 3.63            16    5.13
    adam            u * (|p0| + k * lr)    after k steps                                      2.74            16    2.74

    (measured on an MI355X, ROCm 7.0, torch 2.10; "kernel max" is the HIP kernel's own worst value in the same units, for the
    record only -- no constant is derived from it.  dlogits: the kernel's error never leaves the bf16 ulp of its output.  gelu and
    gelu' sit above their yardstick because the kernels use the Abramowitz-Stegun 7.1.26 erf (absolute error 1.5e-7 = 2.5 u) and
    __expf; still well inside C.)

    Notes on the forms.  mean_row(ax), mean|g| and mean|g xhat| instead of |mean|, |s1| and |s2|: a row sum that cancels is still
    only as good as the sum of its magnitudes.  ax instead of |t|: t is a sum of up to three addends rounded once each, so its rounding scales with
    the addends, not with their sum.  rstd: a perturbation d_i <= u ax_i of the elements moves var by at most 2 std max(d), i.e.
    rstd relatively by u rstd max(ax).  dlogits: the term (p + onehot) rather than |ref| = |p - onehot| because the label's element
    cancels (p -> 1), and + |lse| because row_lse itself is only good to u |lse| and shifts every p of its row relatively by that.
    Adam's test data keeps |g| and |p0| >= 0.25 with equal signs: an element whose clipped gradient (plus weight decay) happens to
    cancel to less than eps = 1e-8 has an update that is discontinuous in the last bit of the clip factor, in any implementation.

Guards: every output buffer has extra rows (and extra columns where the entry point takes a leading dimension) prefilled with
the NaN bit patterns of test_gpu_gemm_routes.py, which must survive; inputs with a leading dimension carry NaN in their padding
columns; every workspace is NaN-filled before a call that folds it (the fold must read only what its first kernel wrote).
Determinism: sumsq, the loss, dgamma / dbeta / dysum and colsum are run twice at their largest case with a different workspace
prefill in between and must agree bit for bit.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import rowop_cases as RC
from tests.dropout_replay import row_mask
from tests.gpu_refs import ref_adam, ref_ce, ref_dgelu, ref_gelu, ref_ln_bwd, ref_ln_fwd, ref_ln_materialize

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
U = 2.0 ** -24
BF_ULP = 2.0 ** -8                       # a full bf16 ulp relative (twice the RNE error: covers a flipped rounding)
SENT = {F32: 0x7FC0DEAD, BF16: 0x7FA5}   # NaN bit patterns (as in test_gpu_gemm_routes.py)
IVIEW = {F32: torch.int32, BF16: torch.int16}
FLT_MIN = 2.0 ** -126                    # smallest normal fp32 (and bf16) number
G = 8                                    # guard rows / elements
SEED = 0x5EED1234
EPS = 1e-7

# The constants of (c): every value equals the table in the module docstring (4 x yardstick maximum, rounded up to a power of 2)
C_LN_T, C_LN_MEAN, C_LN_RSTD, C_LN_OUT, C_LN_MAT = 16.0, 16.0, 4.0, 16.0, 8.0
C_LNB_DT = 16.0
C_LSE, C_DLOGITS = 8.0, 8.0
C_GELU, C_DGELU = 16.0, 16.0
C_ADAM = 16.0


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


# ------------------------------------------------------------------------------------------------ buffers and judging
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * scale


def randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV)


def sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(IVIEW[dtype]).fill_(SENT[dtype])
    return t


def guarded(rows, cols, dtype, ld=None, fill=None, col0=0):
    """[rows + G, ld] of sentinels; returns (full, view [rows, cols] starting at column col0), the view prefilled with `fill`"""
    ld = cols if ld is None else ld
    full = sentinel((rows + G, ld), dtype)
    view = full[:rows, col0:col0 + cols]
    if fill is not None:
        view.copy_(fill)
    return full, view


def guard_intact(full, rows, cols, col0=0):
    bits = full.view(IVIEW[full.dtype])
    s = SENT[full.dtype]
    return bool((bits[rows:] == s).all()) and bool((bits[:rows, :col0] == s).all()) and bool((bits[:rows, col0 + cols:] == s).all())


def guarded1(n, dtype, fill=None):
    full = sentinel((n + G,), dtype)
    if fill is not None:
        full[:n] = fill
    return full, full[:n]


def guard1_intact(full, n):
    return bool((full.view(IVIEW[full.dtype])[n:] == SENT[full.dtype]).all())


def padded_input(vals, ld, dtype=None):
    """[rows, cols] view with row stride ld whose padding columns hold NaN"""
    dtype = dtype or vals.dtype
    rows, cols = vals.shape
    full = sentinel((rows, ld), dtype)
    full[:, :cols] = vals.to(dtype)
    return full[:, :cols]


def nan_ws(ws, value=None):
    if value is None:
        ws.view(torch.int32).fill_(SENT[F32])
    else:
        ws.fill_(value)
    return ws


def worst(err, form):
    """max over elements of err / form; an element whose form is 0 must have err 0"""
    r = torch.where(form > 0, err / form.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def first_bad(bad):
    return tuple(bad.nonzero()[0].tolist())


def judge(what, got, ref, form, C, yard=None, extra=None, floor=0.0):
    """(c): yardstick within C / 4 (when given), kernel within C, in units of `form`; `extra` is an additive allowance of the
    kernel's output format (bf16 ulp), `floor` an absolute one that any fp32 evaluation needs (underflow)"""
    ref = ref.double()
    form = form.double().expand_as(ref)
    ky = None
    if yard is not None:
        ky = worst(((yard.double() - ref).abs() - floor).clamp(min=0.0), form)
    err = ((got.double() - ref).abs() - floor).clamp(min=0.0)
    if extra is not None:
        err = (err - extra.double()).clamp(min=0.0)
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    kk = worst(err, form)
    print(f"[rowops] {what}: yardstick {ky if ky is None else round(ky, 3)} kernel {kk:.3f} C {C}")
    if ky is not None:
        assert ky <= C / 4, f"{what}: the fp32 torch yardstick is {ky:.2f} > C/4 = {C / 4} in units of the form: the reference or the case is off"
    if not kk <= C:
        bad = ~(err <= C * form)
        i = first_bad(bad)
        pytest.fail(f"{what}: kernel error {kk:.2f} > C = {C} in units of the form (yardstick {ky}); {int(bad.sum())} bad elements, "
                    f"first at {i}: got {got[i].item()!r} ref {ref[i].item()!r} form {form[i].item():.3e}")


def exact(what, got, want):
    """bit equality (+0 / -0 are the same value)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = got.view(IVIEW.get(got.dtype, got.dtype)) != want.view(IVIEW.get(want.dtype, want.dtype))
    bad &= ~((got == 0) & (want == 0))
    if bool(bad.any()):
        i = first_bad(bad)
        pytest.fail(f"{what}: {int(bad.sum())} elements differ, first at {i}: got {got[i].item()!r} want {want[i].item()!r}")


def within(what, got, ref, bound):
    """(b): a derived bound"""
    err = (got.double() - ref.double()).abs()
    bad = ~(err <= bound)
    print(f"[rowops] {what}: max err/bound {worst(err, bound.double().expand_as(err)):.3e}")
    if bool(bad.any()):
        i = first_bad(bad)
        pytest.fail(f"{what}: {int(bad.sum())} elements outside the derived bound, first at {i}: got {got[i].item()!r} "
                    f"ref {ref[i].item()!r} bound {bound.expand_as(err)[i].item():.3e}")


def same_zeros(what, got, ref):
    """the zero pattern of a dropout output against the replayed mask (where the reference is not itself 0 by its input)"""
    bad = (got == 0) != (ref == 0)
    assert not bool(bad.any()), f"{what}: zero pattern differs from the replayed keep mask at {int(bad.sum())} elements, first {first_bad(bad)}"


def keep_mask(shape, p):
    return row_mask(SEED, shape, p).to(DEV) if p > 0 else None


# ------------------------------------------------------------------------------------------------ LayerNorm data
def ln_kinds(N):
    """row kinds: 1 common offset +50, 2 scaled by 1e-3, 3 constant except one element, anything else unit normal"""
    r = torch.arange(N, device=DEV)
    return (r + 1) % 8 if N >= 8 else r + 1


def ln_rows(g, N, H):
    x = randn(g, N, H)
    k = ln_kinds(N)[:, None]
    nc = torch.full((H,), 0.7, device=DEV)
    nc[5] = 1.7
    x = torch.where(k == 1, x + 50.0, x)
    x = torch.where(k == 2, x * 1e-3, x)
    return torch.where(k == 3, nc[None].expand(N, H), x).contiguous()


def ln_minor(g, N, H):
    """a small second addend that leaves the near-constant rows alone"""
    return torch.where(ln_kinds(N)[:, None] == 3, torch.zeros((), device=DEV), randn(g, N, H, scale=0.1)).contiguous()


def ln_affine(g, H):
    return (1 + 0.1 * randn(g, H)).contiguous(), (0.1 * randn(g, H)).contiguous()


def ln_rowmask(N):
    return (torch.arange(N, device=DEV) % 5 != 0).to(I32)  # (row 0: a fully masked row)


def torch_ln_stats(t, gamma, beta):
    """torch's own fp32 LayerNorm statistics of t as the [N, 2] (mean, rstd) tensor the kernels take"""
    _, mean, rstd = torch.native_layer_norm(t, (t.shape[1],), gamma, beta, EPS)
    return torch.stack([mean.reshape(-1), rstd.reshape(-1)], 1).contiguous()


# ------------------------------------------------------------------------------------------------ LN forward
LN_FWD = RC.ln_fwd_cases()


@pytest.mark.parametrize("case", LN_FWD, ids=RC.ids(LN_FWD))
def test_ln_fwd(L, case):
    c = case
    N, H = c.N, c.H
    g = gen(1)
    big, small = ln_rows(g, N, H), ln_minor(g, N, H)
    gamma, beta = ln_affine(g, H)
    yv = r = None
    if c.y and c.r_plain:
        r, yv = big, small
    elif c.y:
        yv = big
    else:
        r = big
    y = None
    if c.y == "slice":  # columns [32, 32 + H) of a NaN-filled [N, H + 64] buffer: ldy = H + 64
        y = sentinel((N, H + 64), F32)[:, 32:32 + H]
        y.copy_(yv)
    elif c.y:
        y = yv
    r_norm = None
    if c.r_norm:
        rt = (randn(g, N, H, scale=2.0) + 1.0).contiguous()
        rg, rb = ln_affine(g, H)
        rs = torch_ln_stats(rt, rg, rb)
        rm = None
        if c.r_norm == "masked":
            rm = ((torch.arange(N, device=DEV) % 3 != 0) & (ln_kinds(N) != 3)).to(I32)
        r_norm = (rt, rs, rg, rb, rm)
    rowmask = ln_rowmask(N) if c.rowmask else None
    keep = keep_mask((N, H), c.p) if c.y else None
    ref = ref_ln_fwd(y=y, keep=keep, r_plain=r, r_norm=r_norm, gamma=gamma, beta=beta, eps=EPS, rowmask=rowmask)
    # the fp32 torch yardstick
    t32 = torch.zeros(N, H, device=DEV)
    if y is not None:
        t32 = y * keep if keep is not None else y.clone()
    if r is not None:
        t32 = t32 + r if y is not None else r.clone()
    if r_norm is not None:
        term = (rt - rs[:, :1]) * rs[:, 1:] * rg[None] + rb[None]
        t32 = t32 + (term * rm[:, None].float() if rm is not None else term)
    o32, m32, s32 = torch.native_layer_norm(t32, (H,), gamma, beta, EPS)
    if rowmask is not None:
        o32 = o32 * rowmask[:, None].float()
    # the kernel
    tf, t = guarded(N, H, F32)
    sf, st = guarded(N, 2, F32)
    bfull, ob = guarded(N, H, BF16) if "bf16" in c.outs else (None, None)
    ffull, of = guarded(N, H, F32) if "f32" in c.outs else (None, None)
    L.ln_fwd(y=y, p_drop=c.p, seed=SEED, r_plain=r, r_norm=r_norm, gamma=gamma, beta=beta, eps=EPS, rowmask=rowmask, out_t=t,
             out_stats=st, out_bf16=ob, out_f32=of, N=N, H=H)
    torch.cuda.synchronize()
    for name, full, cols in (("out_t", tf, H), ("out_stats", sf, 2), ("out_bf16", bfull, H), ("out_f32", ffull, H)):
        assert full is None or guard_intact(full, N, cols), f"{c.name} {name}: wrote past row {N}"
    ax = ref["ax"]
    axm = ax.max(1).values
    if c.p == 0 and r_norm is None:
        exact(f"{c.name} out_t", t, t32)  # one fp32 addition (or a copy)
    else:
        judge(f"ln_fwd t {c.name}", t, ref["t"], U * ax, C_LN_T, yard=t32)
    if keep is not None and r is None and r_norm is None:
        same_zeros(f"{c.name} out_t", t, ref["t"])
    judge(f"ln_fwd mean {c.name}", st[:, 0], ref["mean"], U * axm, C_LN_MEAN, yard=m32.reshape(-1))
    judge(f"ln_fwd rstd {c.name}", st[:, 1], ref["rstd"], U * ref["rstd"] * (1 + ref["rstd"] * axm), C_LN_RSTD, yard=s32.reshape(-1))
    om = rowmask.double()[:, None] if rowmask is not None else 1.0
    form = U * (gamma.double().abs()[None] * ref["rstd"][:, None] * (ax + ax.mean(1, keepdim=True)) + ref["out"].abs()) * om
    if of is not None:
        judge(f"ln_fwd out {c.name} f32", of, ref["out"], form, C_LN_OUT, yard=o32)
    if ob is not None:
        judge(f"ln_fwd out {c.name} bf16", ob, ref["out"], form, C_LN_OUT, yard=o32, extra=BF_ULP * ref["out"].abs())
    if of is not None and ob is not None:
        exact(f"{c.name} bf16 output = RNE of the fp32 output", ob, of.to(BF16))


LN_MAT = RC.ln_mat_cases()


@pytest.mark.parametrize("case", LN_MAT, ids=RC.ids(LN_MAT))
def test_ln_materialize(L, case):
    c = case
    N, H = c.N, c.H
    g = gen(2)
    t = ln_rows(g, N, H)
    gamma, beta = ln_affine(g, H)
    st = torch_ln_stats(t, gamma, beta)
    rowmask = ln_rowmask(N) if c.rowmask else None
    S = c.add_bcast
    pos = randn(g, S, H).contiguous() if S else None
    ref, mag = ref_ln_materialize(t, st, gamma, beta, rowmask, pos, S or 1)
    y32 = (t - st[:, :1]) * st[:, 1:] * gamma[None] + beta[None]
    if rowmask is not None:
        y32 = y32 * rowmask[:, None].float()
    if pos is not None:
        y32 = y32 + pos[torch.arange(N, device=DEV) % S]
    ffull, of = guarded(N, H, F32) if "f32" in c.outs else (None, None)
    bfull, ob = guarded(N, H, BF16) if "bf16" in c.outs else (None, None)
    L.ln_materialize(t, st, gamma, beta, rowmask=rowmask, add_bcast=pos, S=S or 1, out_f32=of, out_bf16=ob)
    torch.cuda.synchronize()
    if of is not None:
        assert guard_intact(ffull, N, H), f"{c.name} out_f32: wrote past row {N}"
        judge(f"ln_materialize {c.name} f32", of, ref, U * mag, C_LN_MAT, yard=y32)
    if ob is not None:
        assert guard_intact(bfull, N, H), f"{c.name} out_bf16: wrote past row {N}"
        judge(f"ln_materialize {c.name} bf16", ob, ref, U * mag, C_LN_MAT, yard=y32, extra=BF_ULP * ref.abs())
    if of is not None and ob is not None:
        exact(f"{c.name} bf16 output = RNE of the fp32 output", ob, of.to(BF16))


# ------------------------------------------------------------------------------------------------ LN backward
LN_BWD = RC.ln_bwd_cases()


def sum_bound(terms_abs, n, total):
    """(b): 2 n u sum|term| + 2u |result| (the final += into the accumulator)"""
    return 2.0 * n * U * terms_abs + 2.0 * U * total.abs()


@pytest.mark.parametrize("case", LN_BWD, ids=RC.ids(LN_BWD))
def test_ln_bwd(L, case):
    c = case
    N, H = c.N, c.H
    cap = RC.caps().LNB_BLOCKS
    g = gen(3)
    t = ln_rows(g, N, H)
    gamma, beta = ln_affine(g, H)
    rowmask = ln_rowmask(N) if c.rowmask else None
    dout = (randint(g, -2, 2, N, H).float() if c.int_dout else randn(g, N, H)).contiguous()
    keep = keep_mask((N, H), c.p)
    # statistics: torch's own fp32 ones; yardstick: autograd through the same torch LayerNorm
    tt = t.clone().requires_grad_(True)
    o32, m32, s32 = torch.native_layer_norm(tt, (H,), gamma, beta, EPS)
    st = torch.stack([m32.detach().reshape(-1), s32.detach().reshape(-1)], 1).contiguous()
    (dt32,) = torch.autograd.grad(o32, tt, dout * rowmask[:, None].float() if rowmask is not None else dout)
    dy32 = dt32 * keep if keep is not None else dt32
    ref = ref_ln_bwd(dout, t, st, gamma, rowmask, keep)
    # the kernel
    dtf, dt = guarded(N, H, F32) if c.out_dt else (None, None)
    outs = {}
    if "bf16" in c.dy:
        outs["bf16"] = guarded(N, H, BF16) + (0,)
    if "bf16_wide" in c.dy:
        outs["bf16_wide"] = guarded(N, H, BF16, ld=H + 192 + 8) + (0,)  # the [dy | dz] operand: dy in its first H columns
    dyb = outs["bf16"][1] if "bf16" in outs else (outs["bf16_wide"][1] if "bf16_wide" in outs else None)
    dyff, dyf = guarded(N, H, F32) if "f32" in c.dy else (None, None)
    acc0 = {k: randint(g, -3, 3, H).float() for k in ("dgamma", "dbeta", "dysum")}

    def call(ws_fill):
        acc = {k: guarded1(H, F32, fill=acc0[k]) for k in c.fold}
        ws = nan_ws(L.ln_bwd_ws(H, DEV), ws_fill)
        L.ln_bwd(dout, t, st, gamma, rowmask=rowmask, p_drop=c.p, seed=SEED, out_dt=dt, out_dy_bf16=dyb, out_dy_f32=dyf,
                 dgamma=acc["dgamma"][1] if "dgamma" in acc else None, dbeta=acc["dbeta"][1] if "dbeta" in acc else None,
                 dysum=acc["dysum"][1] if "dysum" in acc else None, ws=ws)
        torch.cuda.synchronize()
        return acc

    acc = call(None)
    where = (f"{c.name} [{RC.ln_bwd_kernel(c.H)}_kernel<{H // 64}>, {RC.ln_bwd_nblk(N, H, cap)} blocks x "
             f"{RC.ln_bwd_iters(N, H, cap)} iterations]")
    if dt is not None:
        assert guard_intact(dtf, N, H), f"{where} out_dt: wrote past row {N}"
        judge(f"ln_bwd dt {where}", dt, ref["dt"], U * ref["mag"], C_LNB_DT, yard=dt32)
    kd = keep.double() if keep is not None else 1.0
    for name, (full, view, col0) in outs.items():
        assert guard_intact(full, N, H, col0), f"{where} out_dy_{name}: wrote outside its [N, H] block"
        judge(f"ln_bwd dy {where} {name}", view, ref["dy"], U * ref["mag"] * kd, C_LNB_DT, yard=dy32, extra=BF_ULP * ref["dy"].abs())
        if keep is not None:
            assert bool((view[keep == 0] == 0).all()), f"{where} dy {name}: a dropped element is not zero"
    if dyf is not None:
        assert guard_intact(dyff, N, H), f"{where} out_dy_f32: wrote past row {N}"
        judge(f"ln_bwd dy {where} f32", dyf, ref["dy"], U * ref["mag"] * kd, C_LNB_DT, yard=dy32)
        if keep is not None:
            assert bool((dyf[keep == 0] == 0).all()), f"{where} dy f32: a dropped element is not zero"
        if dt is not None:
            exact(f"{where} dy = dt * keep (one fp32 multiplication)", dyf, dt * keep if keep is not None else dt)
        if dyb is not None:
            exact(f"{where} bf16 dy = RNE of the fp32 dy", dyb.contiguous(), dyf.to(BF16))
    # the column sums, judged on their own
    for k in c.fold:
        assert guard1_intact(acc[k][0], H), f"{where} {k}: wrote past H"
    if "dbeta" in c.fold:
        total = acc0["dbeta"].double() + ref["tb"].sum(0)
        if c.int_dout:
            exact(f"{where} dbeta (integer dout: exact)", acc["dbeta"][1], total.float())
        else:
            within(f"{where} dbeta", acc["dbeta"][1], total, sum_bound(ref["tb"].abs().sum(0), N, total))
    if "dgamma" in c.fold:
        total = acc0["dgamma"].double() + ref["tg"].sum(0)
        std = st.double()
        # the three fp32 roundings of a term dout * (t - mean) * rstd before it is summed (module docstring, (b))
        term_round = 4.0 * U * (ref["tb"].abs() * std[:, 1:] * (t.double().abs() + std[:, :1].abs())).sum(0)
        within(f"{where} dgamma", acc["dgamma"][1], total, sum_bound(ref["tg"].abs().sum(0), N, total) + term_round)
    if "dysum" in c.fold:
        terms = dyf.double() if dyf is not None else dt.double() * kd
        total = acc0["dysum"].double() + terms.sum(0)
        within(f"{where} dysum", acc["dysum"][1], total,
               sum_bound(terms.abs().sum(0), N, total) + (0.0 if dyf is not None else 2.0 * U * terms.abs().sum(0)))
    if c.twice:
        acc2 = call(12345.0)
        for k in c.fold:
            assert torch.equal(acc[k][0].view(torch.int32), acc2[k][0].view(torch.int32)), f"{where} {k}: not reproducible bit for bit"


# ------------------------------------------------------------------------------------------------ cross entropy
CE = RC.ce_cases()
GSCALE = 0.37


def ce_inputs(c):
    g = gen(4)
    N, V = c.N, c.V
    x = randn(g, N, V, scale=3.0)
    x[0] = 2.5                      # all-equal logits
    x[1, V - 1] += 80.0             # a maximum far above the rest in the last element any thread sees
    x[3] = x[3] * 10.0
    x[4, V - 1] += 80.0             # ... with the label elsewhere
    x[6, (V // 2) | 3] += 80.0      # ... in the middle of a row
    labels = randint(g, 0, V - 1, N)
    labels[torch.arange(N, device=DEV) % 3 == 2] = -100
    labels[0], labels[1], labels[3], labels[4], labels[6] = 0, V - 1, V - 1, 0, 7
    return padded_input(x, c.ld), labels


@pytest.mark.parametrize("case", CE, ids=RC.ids(CE))
def test_cross_entropy(L, case):
    c = case
    N, V, Vp = c.N, c.V, c.Vp
    logits, labels = ce_inputs(c)
    ref = ref_ce(logits, labels)
    on = ref["on"]

    def fwd():
        lf, lse = guarded1(N, F32)
        af, acc = guarded1(2, F32, fill=0.0)
        L.ce_fwd(logits, labels, V, lse, acc)
        torch.cuda.synchronize()
        return lf, lse, af, acc

    lf, lse, af, acc = fwd()
    assert guard1_intact(lf, N) and guard1_intact(af, 2), f"{c.name}: ce_fwd wrote past its outputs"
    assert bool((lse[~on] == 0).all()), f"{c.name}: row_lse of an ignored row is not 0"
    lse32 = torch.logsumexp(logits.contiguous(), 1)
    judge(f"ce row_lse {c.name}", lse[on], ref["lse"][on], U * ref["lse"][on].abs().clamp(min=1.0), C_LSE, yard=lse32[on])
    assert acc[1].item() == ref["count"], f"{c.name}: count {acc[1].item()} != {ref['count']}"
    # (b) the loss sum on its own: the kernel's row_lse as terms, each lse - logit[label] rounded once, then at most N additions
    xl = ref["x"].gather(1, labels.clamp(min=0)[:, None])[:, 0]
    terms = torch.where(on, lse.double() - xl, torch.zeros_like(xl))
    within(f"{c.name} loss sum", acc[0], terms.sum(), 2.0 * (ref["count"] + 1) * U * terms.abs().sum())
    if c.twice:
        _, lse2, _, acc2 = fwd()
        assert torch.equal(acc, acc2) and torch.equal(lse, lse2), f"{c.name}: loss not reproducible bit for bit"
    # backward on a row list
    lab_rows = torch.nonzero(on).view(-1)
    ign_rows = torch.nonzero(~on).view(-1)
    if c.rows == "padded":  # a fixed-capacity list: ignored entries in between, the tail padded with one repeated ignored row
        rows = torch.cat([lab_rows[:5], ign_rows[:2], lab_rows[5:], ign_rows[-1:].repeat(11)])
    else:
        rows = lab_rows
    R = rows.numel()
    rows32 = rows.to(I32)
    gs = torch.tensor([GSCALE], device=DEV) if c.gscale == "tensor" else GSCALE
    df, d = guarded(R, Vp, BF16)
    L.ce_bwd_rows(logits, labels, rows32, V, Vp, lse, acc, gs, d)
    torch.cuda.synchronize()
    assert guard_intact(df, R, Vp), f"{c.name}: ce_bwd_rows wrote past row {R}"
    assert bool((d[:, V:] == 0).all()), f"{c.name}: columns [V, Vp) are not exactly zero"
    ron = on[rows]
    assert bool((d[~ron] == 0).all()), f"{c.name}: an ignored row of the list has a nonzero gradient"
    sc = float(torch.tensor(GSCALE, dtype=F32)) / max(ref["count"], 1)
    xr = ref["x"][rows[ron]]
    lr_ = ref["lse"][rows[ron]][:, None]
    p = torch.exp(xr - lr_)
    onehot = torch.zeros_like(p).scatter_(1, labels[rows[ron]][:, None], 1.0)
    dref = (p - onehot) * sc
    form = U * (p + onehot) * ((xr - lr_).abs().clamp(min=1.0) + lr_.abs()) * sc
    del xr
    x32 = logits.contiguous().requires_grad_(True)
    (g32,) = torch.autograd.grad(F.cross_entropy(x32, labels, ignore_index=-100), x32)
    yard = g32[rows[ron]] * GSCALE
    del g32, x32
    # (floor: a probability times the scale below fp32's normal range -- rows scaled by 10 reach exp(-250) -- underflows)
    judge(f"ce dlogits {c.name}", d[ron][:, :V], dref, form, C_DLOGITS, yard=yard, extra=BF_ULP * dref.abs(), floor=FLT_MIN)


# ------------------------------------------------------------------------------------------------ sumsq / Adam
SS = RC.sumsq_cases()


@pytest.mark.parametrize("case", SS, ids=RC.ids(SS))
def test_sumsq(L, case):
    c = case
    g = gen(5)
    nws = L.load().fbl_sumsq_ws_floats()
    x = randint(g, -4, 4, c.n).float() if c.exact else randn(g, c.n)

    def call(fill):
        wf, ws = guarded1(nws, F32)
        nan_ws(ws, fill)
        of, out = guarded1(1, F32, fill=3.0)
        L.sumsq(x, out, ws=ws)
        torch.cuda.synchronize()
        assert guard1_intact(wf, nws) and guard1_intact(of, 1), f"{c.name}: wrote past ws / out"
        return out.clone()

    out = call(None)
    sq = x.double() ** 2
    total = 3.0 + sq.sum()
    if c.exact:
        exact(f"{c.name} (integers: exact)", out, total.float().reshape(1))
    else:
        within(f"{c.name}", out, total.reshape(1), (2.0 * c.n * U * sq.sum() + 2.0 * U * total).reshape(1))
    if c.twice:
        assert torch.equal(out, call(7.0)), f"{c.name}: not reproducible bit for bit"


ADAM = RC.adam_cases()
LR, B1, B2, AEPS = 3e-4, 0.9, 0.95, 1e-8


@pytest.mark.parametrize("case", ADAM, ids=RC.ids(ADAM))
def test_adam(L, case):
    c = case
    n = c.n
    g_ = gen(6)
    sign = (randint(g_, 0, 1, n) * 2 - 1).float()
    # |g|, |p0| >= 0.25 with equal signs (see the module docstring); a fresh gradient every step: with the same one m / sqrt(v) is
    # +-1 whatever its size, and neither weight decay nor the clip factor would show in p
    grads = [(sign * (0.25 + randn(g_, n).abs())).contiguous() for _ in c.steps]
    p0 = (sign * (0.25 + randn(g_, n).abs())).contiguous()
    norms = [math.sqrt(float((gr.double() ** 2).sum())) * c.grad_scale for gr in grads]
    max_norm = {"none": 0.0, "below": 0.5 * min(norms), "above": 2.0 * max(norms)}[c.max_norm]
    clips = [c.grad_scale * (min(1.0, max_norm / (nm + 1e-6)) if max_norm > 0 else 1.0) for nm in norms]
    assert all((c.max_norm == "below") == (cl < c.grad_scale) for cl in clips)
    # a run that starts late (step 1000) starts from moments of the size the earlier steps would have left
    late = c.steps[0] != 1
    m0 = (sign * 0.05 * (0.25 + randn(g_, n).abs()) * clips[0]).contiguous() if late else torch.zeros(n, device=DEV)
    v0 = ((0.05 * (0.25 + randn(g_, n).abs()) * clips[0]) ** 2).contiguous() if late else torch.zeros(n, device=DEV)
    # float64 reference and the fp32 torch yardstick
    p64, m64, v64 = p0.double(), m0.double(), v0.double()
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pt], lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=c.wd)
    if late:
        opt.state[pt] = dict(step=torch.tensor(float(c.steps[0] - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    pf, p = guarded1(n, F32, fill=p0)
    mf, m = guarded1(n, F32, fill=m0)
    vf, v = guarded1(n, F32, fill=v0)
    ss = torch.zeros(1, device=DEV)
    nws = L.load().fbl_sumsq_ws_floats()
    for step, grad, clip in zip(c.steps, grads, clips):
        ref_adam(p64, grad.double(), m64, v64, lr=LR, b1=B1, b2=B2, eps=AEPS, wd=c.wd, step=step, clip=clip)
        pt.grad = grad * c.grad_scale
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        ss.zero_()
        L.sumsq(grad, ss, ws=nan_ws(torch.empty(nws, device=DEV)))
        L.adam_flat(p, grad, m, v, LR, B1, B2, AEPS, c.wd, step, sumsq_t=ss, max_norm=max_norm, grad_scale=c.grad_scale)
    torch.cuda.synchronize()
    assert guard1_intact(pf, n) and guard1_intact(mf, n) and guard1_intact(vf, n), f"{c.name}: wrote past n"
    judge(f"adam p {c.name}", p, p64, U * (p0.double().abs() + len(c.steps) * LR), C_ADAM, yard=pt.detach())
    # (sanity, not a tolerance: |m / sqrt(v)| of these gradients is above 0.1 at every step, so every element moves by > 0.1 lr)
    moved = (p.double() - p0.double()).abs()
    assert float(moved.min()) > 0.1 * LR, f"{c.name}: an element did not move"


# ------------------------------------------------------------------------------------------------ column sums
CS = RC.colsum_cases()


@pytest.mark.parametrize("case", CS, ids=RC.ids(CS))
def test_colsum(L, case):
    c = case
    rows, cols = c.rows, c.cols
    width = c.width or cols
    ld = c.ld or width
    dt = BF16 if c.bf16 else F32
    g = gen(7)
    for exact_pass in (True, False):
        vals = randint(g, -4, 4, rows, width).float() if exact_pass else randn(g, rows, width).to(dt).float()
        x = padded_input(vals, ld, dt)
        acc0 = randint(g, -5, 5, cols).float()

        def call(fill):
            of, out = guarded1(cols, F32, fill=acc0)
            ws = nan_ws(L.colsum_ws(cols, DEV), fill)
            L.colsum(x, out, ws, rows=rows, cols=cols)
            torch.cuda.synchronize()
            assert guard1_intact(of, cols), f"{c.name}: wrote past column {cols}"
            return out.clone()

        out = call(None)
        v = x[:, :cols].double()
        total = acc0.double() + v.sum(0)
        if exact_pass:
            exact(f"{c.name} (integers: exact)", out, total.float())
        else:
            within(f"{c.name}", out, total, sum_bound(v.abs().sum(0), rows, total))
            if c.twice:
                assert torch.equal(out, call(-3.0)), f"{c.name}: not reproducible bit for bit"


# ------------------------------------------------------------------------------------------------ element-wise kernels
ELEM = RC.elem_cases()


def gelu_inputs(g, n):
    """unit normals x 2, every 7th element in the tails 6 <= |c| <= 12, a few exact zeros and far values"""
    c = randn(g, n, scale=2.0)
    i = torch.arange(n, device=DEV)
    tail = (6.0 + 6.0 * torch.rand(n, generator=g, device=DEV)) * torch.where(i % 14 == 0, 1.0, -1.0)
    c = torch.where(i % 7 == 0, tail, c)
    c = torch.where(i % 1001 == 5, torch.zeros((), device=DEV), c)
    return torch.where(i % 1001 == 6, torch.where(i % 2 == 0, 30.0, -30.0), c).contiguous()


def cast_inputs(g, n):
    x = randn(g, n) * torch.exp(randn(g, n, scale=8.0))
    i = torch.arange(n, device=DEV)
    b = torch.randint(0, 0x7F80, (n,), generator=g, device=DEV, dtype=torch.int32)         # a finite non-negative bf16 pattern
    tie = ((b << 16) | 0x8000) | torch.where(i % 2 == 0, 0, -0x80000000).to(torch.int32)   # exactly half way to the next one
    x = torch.where(i % 5 == 1, tie.view(F32), x)
    den = torch.randint(1, 0x7FFFFF, (n,), generator=g, device=DEV, dtype=torch.int32)     # fp32 denormals
    x = torch.where(i % 5 == 2, den.view(F32), x)
    special = torch.tensor([0.0, -0.0, math.inf, -math.inf, 3.3895314e38, 3.4028235e38, 1e-40, -1e-45], device=DEV)
    k = min(n, special.numel())
    if n >= 16:
        x[8:8 + k] = special[:k]
    return x.contiguous()


@pytest.mark.parametrize("case", ELEM, ids=RC.ids(ELEM))
def test_elementwise(L, case):
    c = case
    n, p = c.n, c.p
    g = gen(8)
    keep = row_mask(SEED, (1, n), p).view(-1).to(DEV) if p > 0 else None
    kd = keep.double() if keep is not None else 1.0
    if c.op == "gelu_fwd":
        x = gelu_inputs(g, n)
        of, out = guarded1(n, F32)
        L.dropout_gelu_fwd(x, p, SEED, out)
        torch.cuda.synchronize()
        assert guard1_intact(of, n), f"{c.name}: wrote past n"
        v = x.double() * kd
        judge(f"gelu {c.name}", out, ref_gelu(v), U * v.abs(), C_GELU, yard=F.gelu(x * keep if keep is not None else x))
    elif c.op == "gelu_bwd":
        x = gelu_inputs(g, n)
        dy = randn(g, n).contiguous()
        of, out = guarded1(n, F32)
        bfull, ob = guarded1(n, BF16)
        L.dropout_gelu_bwd(dy, x, p, SEED, out_bf16=ob, out_f32=out)
        torch.cuda.synchronize()
        assert guard1_intact(of, n) and guard1_intact(bfull, n), f"{c.name}: wrote past n"
        d = ref_dgelu(x.double() * kd)
        ref = dy.double() * d * kd
        form = U * dy.double().abs() * kd * d.abs().clamp(min=1.0)
        xr = x.clone().requires_grad_(True)
        (yard,) = torch.autograd.grad(F.gelu(xr * keep if keep is not None else xr), xr, dy)
        judge(f"gelu' {c.name} f32", out, ref, form, C_DGELU, yard=yard)
        judge(f"gelu' {c.name} bf16", ob, ref, form, C_DGELU, yard=yard, extra=BF_ULP * ref.abs())
        exact(f"{c.name} bf16 output = RNE of the fp32 output", ob, out.to(BF16))
        if keep is not None:
            assert bool((out[keep == 0] == 0).all()) and bool((ob[keep == 0] == 0).all()), f"{c.name}: a dropped element is not zero"
            # the forward draws the same mask: dropped there <=> dropped here
            ff, fwd = guarded1(n, F32)
            L.dropout_gelu_fwd(torch.full((n,), 3.0, device=DEV), p, SEED, fwd)
            assert bool(((fwd == 0) == (keep == 0)).all()), f"{c.name}: forward and backward masks differ"
    elif c.op == "dropout_f32":
        x = randn(g, n).contiguous()
        of, out = guarded1(n, F32)
        bfull, ob = guarded1(n, BF16)
        L.dropout_f32(x, p, SEED, out_f32=out, out_bf16=ob)
        torch.cuda.synchronize()
        assert guard1_intact(of, n) and guard1_intact(bfull, n), f"{c.name}: wrote past n"
        want = x * keep if keep is not None else x
        exact(f"{c.name} f32 (one fp32 multiplication)", out, want)
        exact(f"{c.name} bf16", ob, want.to(BF16))
        same_zeros(c.name, out, want)
    elif c.op == "dropout_bf16":
        x = randn(g, n).to(BF16)
        full, xb = guarded1(n, BF16, fill=x)
        L.dropout_bf16_(xb, p, SEED)
        torch.cuda.synchronize()
        assert guard1_intact(full, n), f"{c.name}: wrote past n"
        want = (x.float() * keep).to(BF16)
        exact(c.name, xb, want)
        same_zeros(c.name, xb, want)
        L.dropout_bf16_(xb, 0.0, SEED)  # p = 0: a no-op by contract
        exact(f"{c.name} then p = 0", xb, want)
    else:
        x = cast_inputs(g, n)
        full, out = guarded1(n, BF16)
        L.cast_bf16(x, out)
        torch.cuda.synchronize()
        assert guard1_intact(full, n), f"{c.name}: wrote past n"
        exact(f"{c.name} (RNE)", out, x.to(BF16))


# ------------------------------------------------------------------------------------------------ gather / scatter rows
ROWS = RC.rows_cases()


@pytest.mark.parametrize("case", ROWS, ids=RC.ids(ROWS))
def test_gather_scatter_rows(L, case):
    c = case
    g = gen(9)
    if c.op == "gather":
        src = padded_input(randn(g, c.src_rows, c.cols), c.cols + 8, BF16)
        rows = randint(g, 0, c.src_rows - 1, c.R).to(I32)
        rows[1::7] = rows[0]  # repeated indices
        full, out = guarded(c.R, c.cols, BF16)
        L.gather_rows_bf16(src, rows, out)
        torch.cuda.synchronize()
        assert guard_intact(full, c.R, c.cols), f"{c.name}: wrote past row {c.R}"
        exact(c.name, out, src[rows.long()].contiguous())
    else:
        upd = randn(g, c.R, c.cols).contiguous()
        rows = torch.randperm(c.src_rows, generator=g, device=DEV)[:c.R].to(I32)
        base = randn(g, c.src_rows, c.cols)
        full, out = guarded(c.src_rows, c.cols, F32, ld=c.cols + 8, fill=base)
        L.scatter_rows_f32(upd, rows, out)
        torch.cuda.synchronize()
        assert guard_intact(full, c.src_rows, c.cols), f"{c.name}: wrote outside [rows, cols]"
        want = base.clone()
        want[rows.long()] += upd
        exact(f"{c.name} (one fp32 addition per element)", out.contiguous(), want)
