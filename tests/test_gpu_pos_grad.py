"""fbl_attn_pos_grad (csrc/attn_bwd.hip: pos_grad_kernel, pos_grad_wide_kernel) against its definition in float64.

  dPK[e][h][r][d] = sum_b sum_{(i,j): idx(i-j) = r} dS_b[i,j] Q_b[i,d]     (neg = 0: X = dS,   Y = Q)
  dPQ[e][h][r][d] = sum_b sum_{(i,j): idx(i-j) = r} dS_b[i,j] K_b[j,d]     (neg = 1: X = dS^T, Y = K)

on random bf16 X / Y, with the dlo / dcnt of the call (attn_bwd._delta_ranges).  The bound is the one
tests/test_gpu_kernels.py::test_attention_bwd applies to dPK / dPQ: rtol 3e-2, atol 2e-2 * max |reference|.

Shapes: the smallest at which each path of the kernel can go wrong -- one staged block inside the identity band (S = 37), deltas
across the band's edge at 128 (S = 140, up to 3 deltas per table row), the 332 table rows of S = 266 (21 tiles: more than
16, every tile slot of the workgroup that owns a whole (execution, head)), S = 512 (up to 6 deltas per row, the table split over
two workgroups), and a coarse map (64 buckets) at S = 512 that must reach the prefix-difference kernel.  Ragged lengths
(1, below 32, no multiple of 32, S), the packed row layout of Y, NaN in everything the kernel must not read into a result, and
two identical calls compared bit for bit.
"""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
RTOL, ATOL_REL = 3e-2, 2e-2  # test_attention_bwd: close(dpqk, ref, 3e-2, 2e-2 * max |ref|)

FBL_MAP = dict(position_buckets=256, max_rel=512, att_span=256)  # the FrozenBiLM map
COARSE_MAP = dict(position_buckets=64, max_rel=512, att_span=64)

#        id             S    B  klen                     packed  nan    map
CASES = {
    "s37": (37, 3, None, False, False, FBL_MAP),
    "s140": (140, 4, [140, 1, 17, 75], False, False, FBL_MAP),
    "s140_packed": (140, 4, [75, 140, 1, 17], True, False, FBL_MAP),
    "s266_nan": (266, 4, [266, 1, 20, 100], False, True, FBL_MAP),
    "s266_packed": (266, 4, [100, 266, 20, 1], True, False, FBL_MAP),
    "s512": (512, 2, [512, 200], False, False, FBL_MAP),
    "s512_coarse": (512, 2, [512, 200], False, False, COARSE_MAP),
}
E, NH = 2, 2


def make_case(name):
    """Inputs of a case (device tensors) -- deterministic, shared by the test and by the tools that compare two libraries."""
    from frozenbilm_amd.attn_bwd import _delta_ranges

    S, B, klen, packed, nan, cmap = CASES[name]
    Sp = (S + 63) // 64 * 64
    H = NH * 64
    g = torch.Generator(device="cpu").manual_seed(1000 + S + 7 * len(name))
    kl = klen if klen is not None else [S] * B
    dlo, dcnt, dmax = _delta_ranges(S, types.SimpleNamespace(**cmap), torch.device(DEV), limit=None)
    rcnt = dlo.numel()
    Xs, Ys = [[], []], [[], []]  # [neg][e]
    lens = kl if packed else [S] * B
    row0 = [0]
    for n in lens:
        row0.append(row0[-1] + n)
    for neg in (0, 1):
        for _ in range(E):
            # only the [klen x klen] corner of dS / dS^T is non-zero; the kernel may read the 32-row blocks below klen and the
            # columns below klen rounded up to 64 (zeros, as kernel A writes them) and nothing else
            x = torch.zeros(B, NH, Sp, Sp)
            if nan:
                x.fill_(float("nan"))
            for b in range(B):
                k32, k64 = (kl[b] + 31) // 32 * 32, (kl[b] + 63) // 64 * 64
                x[b, :, :k32, :k64] = 0.0
                x[b, :, :kl[b], :kl[b]] = torch.randn(NH, kl[b], kl[b], generator=g)
            y = torch.randn(row0[-1], 3 * H, generator=g)  # a [rows, 3H] qkv-like tensor: Y is a column slice of it
            Xs[neg].append(x.to(BF16).to(DEV))
            Ys[neg].append(y.to(BF16).to(DEV))
    return dict(S=S, Sp=Sp, B=B, kl=kl, rcnt=rcnt, dmax=dmax, dlo=dlo, dcnt=dcnt, Xs=Xs, Ys=Ys,
                klen=None if klen is None else torch.tensor(klen, dtype=torch.int32, device=DEV),
                row0=torch.tensor(row0, dtype=torch.int32, device=DEV) if packed else None, row0_host=row0)


def run_case(L, c, neg):
    """One fbl_attn_pos_grad call: out [E, NH, rcnt, 64] fp32 (starts NaN-filled: every element must be written)"""
    H = NH * 64
    out = torch.full((E, NH, c["rcnt"], 64), float("nan"), dtype=F32, device=DEV)
    ys = [y[:, neg * H:(neg + 1) * H] for y in c["Ys"][neg]]
    L.attn_pos_grad(neg, c["Xs"][neg], ys, c["dlo"], c["dcnt"], c["dmax"], out, c["B"], c["S"], c["Sp"], NH, c["rcnt"],
                    klen=c["klen"], row0=c["row0"])
    torch.cuda.synchronize()
    return out


def reference(c, neg):
    """float64 on the CPU, straight from the definition.  Returns (out, bound): bound is the per-element derived bound of
    tests/attn_refs.py -- the MFMA operand G[r][k] (the fp32 sum of the <= 8 values of a table row's deltas, or a difference of two
    fp32 prefix sums of the staged row where a row collects more than 8) is rounded to bf16, the sum over k and over the batch is
    an fp32 reduction of n = sum_b klen_b exact products:
        |err| <= (2^-8 + 16 u + 2 n u) sum |G|abs |y|   (+ 96 u sum_k rowabs_k |y_k| for the prefix-difference kernel)"""
    from tests.attn_refs import G_RND, PREFIX_RND, U
    S, B, kl, rcnt = c["S"], c["B"], c["kl"], c["rcnt"]
    H = NH * 64
    dlo, dcnt = c["dlo"].cpu().long(), c["dcnt"].cpu().long()
    row_of = torch.full((2 * S - 1,), -1, dtype=torch.long)  # delta + S - 1 -> table row
    for r in range(rcnt):
        lo, n = int(dlo[r]), int(dcnt[r])
        row_of[lo + S - 1:lo + n + S - 1] = r
    assert (row_of >= 0).all()
    kk = torch.arange(S)
    # X[k][col]: neg = 0 -> k = i, col = j, delta = k - col;  neg = 1 -> k = j, col = i, delta = col - k
    delta = (kk[None, :] - kk[:, None]) if neg else (kk[:, None] - kk[None, :])
    R = row_of[delta + S - 1]  # [k, col]
    out = torch.zeros(E, NH, rcnt, 64, dtype=torch.float64)
    mag = torch.zeros_like(out)
    wide = torch.zeros(E, NH, 1, 64, dtype=torch.float64)
    for e in range(E):
        x = c["Xs"][neg][e].cpu().double()
        y = c["Ys"][neg][e].cpu().double()[:, neg * H:(neg + 1) * H]
        for b in range(B):
            n = kl[b]
            xb = x[b, :, :n, :n]  # [NH, k, col]
            G = torch.zeros(NH, n, rcnt, dtype=torch.float64).scatter_add_(2, R[:n, :n].expand(NH, n, n), xb)
            r0 = c["row0_host"][b]
            yb = y[r0:r0 + n].view(n, NH, 64)
            out[e] += torch.einsum("hkr,khd->hrd", G, yb)
            Ga = torch.zeros(NH, n, rcnt, dtype=torch.float64).scatter_add_(2, R[:n, :n].expand(NH, n, n), xb.abs())
            mag[e] += torch.einsum("hkr,khd->hrd", Ga, yb.abs())
            wide[e] += torch.einsum("hk,khd->hd", xb.abs().sum(2), yb.abs())[:, None, :]
    bound = (G_RND + 2 * sum(kl) * U) * mag
    if c["dmax"] > 8:
        bound = bound + PREFIX_RND * wide
    return out, bound


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


@pytest.mark.parametrize("name", list(CASES))
def test_pos_grad(L, name):
    c = make_case(name)
    if name == "s512_coarse":
        assert c["dmax"] > 8  # the prefix-difference kernel's dispatch rule
    elif name == "s512":
        assert 3 < c["dmax"] <= 8
    else:
        assert c["dmax"] <= 3
    for neg in (0, 1):
        got = run_case(L, c, neg)
        again = run_case(L, c, neg)
        ref, bound = reference(c, neg)
        g = got.cpu().double()
        assert torch.isfinite(g).all(), f"{name} neg={neg}: non-finite results"
        atol = ATOL_REL * ref.abs().max().item()
        err = (g - ref).abs()
        print(f"{name} neg={neg}: max |err| {err.max().item():.3e}  max |ref| {ref.abs().max().item():.3e}  atol {atol:.3e}")
        assert torch.allclose(g, ref, rtol=RTOL, atol=atol), f"{name} neg={neg}: max |err| {err.max().item():.3e}, atol {atol:.3e}"
        assert torch.equal(got, again), f"{name} neg={neg}: two identical calls differ"
        # per element, next to the global bound above: bf16 G operand + fp32 reduction
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
        print(f"{name} neg={neg}: worst |err| / derived bound {ratio.max().item():.3f}")
        assert ratio.max().item() <= 1.0, f"{name} neg={neg}: |err| / bound {ratio.max().item():.3f} at {int(ratio.argmax())}"
