"""Every case of tests/adw_cases.py run through fbl_adapter_bwd_dw on the MI355X and compared, for EVERY adapter of the group, with
a float64 reference computed on the GPU from the very operand bits the kernel gets:

    dWu[H, A] += sum_seg dy^T . z      dWd[A, H] += sum_seg dz^T . x      dbd[A] += sum_seg colsum(dz)

Exact pass (every case).  dy, dz, x are integers in [-2, 2], z in [0, 3], the prefill in [-50, 50]: every partial sum is an integer
below 2^24 (tests/test_adw_cases.py asserts it per case), so each output must equal prefill + reference bit for bit -- a row, a
column, a segment or an adapter in the wrong place cannot hide in a tolerance.  A second launch on fresh prefills gives the same bits.

Random-data pass (one case per instantiation, the LoRA cases, the production case).  Unit normals rounded to bf16 (z: their
positive part, as behind a ReLU), prefill ten times as large.  Per element, with K = segments * N and u = 2^-24,

    |got - ref| <= 2 K u * T + 2 u |ref|        T = (|dy|^T . |z|),  (|dz|^T . |x|)  or  colsum |dz|  summed over the segments,

the form derived in tests/test_gpu_gemm_routes.py: products of two bf16 numbers are exact in fp32; each of the at most K fp32
additions that sum them -- inside an MFMA, between MFMAs, in v_dot2 or in the fold of the column sums' eight partials -- is off by
at most one ulp (2u relative) of a partial sum that T bounds, truncating or rounding; the single addition into the prefill is off
by at most u |result|, taken as 2u |ref|.  There is no other slack.  The test prints the largest err / bound per output.

Group independence (random data).  An adapter's three outputs have the same bits whether it is launched alone, at its place in
the full group, in the group reversed, or in a group of five: a workgroup accumulates one tile of one adapter over all its rows in
a fixed order, whatever the rest of the grid does.  dw_group and the LoRA grouping loop of the engine rely on it.

Buffers.  Operand buffers have 64-row-tile padding rows below N and padding columns beyond H / Ap, all filled with a NaN bit
pattern (columns A .. Ap of z and dz hold zero: the contract); a load outside the operand poisons the output it reaches.  Outputs
are prefilled and followed by guard rows of the pattern, which must survive.
"""
import pytest
import torch

from tests import adw_cases as AC
from tests.test_gpu_gemm_routes import BF16, DEV, F32, IVIEW, SENT, U, Gen, guard_intact, guarded, operand

pytestmark = pytest.mark.gpu

CASES = AC.cases()
GUARD = 64  # sentinel elements around a flat output view


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


# ------------------------------------------------------------------------------------------------ operands
def rows_pad(N):
    """rows of an operand buffer: the row tiles that hold N, and at least one sentinel row"""
    return (N // 64 + 1) * 64


def padded_operand(vals, N, ld):
    """operand() of the helpers with sentinel ROWS below N as well; vals: [N, cols] fp32.  Returns the [N, cols] view."""
    Nr = rows_pad(N)
    v = operand(torch.cat([vals, torch.zeros(Nr - N, vals.shape[1], device=DEV)]), ld)
    v[N:].view(torch.int16).fill_(SENT[BF16])
    return v[:N]


def make_segment(c, g, o, seg):
    """(dy, z, dz, x) of one execution of adapter o, in the layout of the case; `seg` counts the segments of the whole case"""
    N, H, A, Ap = c.N, c.H, c.A, c.Ap
    dy, dz, x = g.val(N, H), g.val(N, A), g.val(N, H)
    z = g.val(N, A, lo=0, hi=3)
    if not g.exact:
        z = torch.relu(z)
    if c.rows != "all":
        gone = torch.ones(N, dtype=torch.bool, device=DEV)
        gone[torch.tensor(AC.row_keep(c, seg), device=DEV)] = False
        dy[gone] = 0
        dz[gone] = 0
    zeros = torch.zeros(N, Ap - A, device=DEV)
    zp, dzp = torch.cat([z, zeros], 1), torch.cat([dz, zeros], 1)
    if c.layout == "lora":
        packed = padded_operand(torch.cat([g.val(N, H), dy, g.val(N, H)], 1), N, 3 * H)  # dy is its middle column block
        return packed[:, H:2 * H], padded_operand(zp, N, Ap), padded_operand(dzp, N, Ap), padded_operand(x, N, H)
    xv, zv = padded_operand(x, N, H + 64), padded_operand(zp, N, Ap + 8)
    if o % 2 == 1:  # folded: [dy | dz | 64 sentinel columns]
        both = padded_operand(torch.cat([dy, dzp], 1), N, H + Ap + 64)
        return both[:, :H], zv, both[:, H:], xv
    return padded_operand(dy, N, H + 64), zv, padded_operand(dzp, N, Ap + 8), xv


def make_adapters(c, exact, seed):
    g = Gen(seed, exact)
    ads, seg = [], 0
    for o, n in enumerate(c.seg_counts):
        ads.append([make_segment(c, g, o, seg + k) for k in range(n)])
        seg += n
    return ads


def make_prefills(c, exact, seed):
    g = Gen(seed, exact)
    return [dict(dWu=g.val(c.H, c.A, lo=-AC.PREFILL_MAX, hi=AC.PREFILL_MAX, scale=10.0),
                 dWd=g.val(c.A, c.H, lo=-AC.PREFILL_MAX, hi=AC.PREFILL_MAX, scale=10.0),
                 dbd=g.val(1, c.A, lo=-AC.PREFILL_MAX, hi=AC.PREFILL_MAX, scale=10.0)) for _ in range(c.adapters)]


# ------------------------------------------------------------------------------------------------ outputs
class Out:
    """one prefilled output with its guards: `view` goes to the kernel"""

    def __init__(self, fill, offset):
        rows, cols = fill.shape
        self.rows, self.cols, self.offset = rows, cols, offset
        if offset:  # a contiguous view at an element offset of a flat buffer (8-byte aligned for offset 2)
            self.full = torch.empty(offset + rows * cols + GUARD, dtype=F32, device=DEV)
            self.full.view(torch.int32).fill_(SENT[F32])
            self.view = self.full[offset:offset + rows * cols].view(rows, cols)
            self.view.copy_(fill)
        else:
            self.full, self.view = guarded(rows, cols, cols, F32, fill)

    def intact(self):
        if self.offset:
            bits = self.full.view(torch.int32)
            n = self.rows * self.cols
            return bool((bits[:self.offset] == SENT[F32]).all()) and bool((bits[self.offset + n:] == SENT[F32]).all())
        return guard_intact(self.full, self.rows, self.cols)


def launch(L, c, ads, pre, order=None):
    """one launch of the adapters `order` (default: all, in order); returns {adapter: {name: Out}}"""
    order = list(range(c.adapters)) if order is None else order
    outs, groups = {}, []
    for o in order:
        mine = {k: Out(pre[o][k], c.out_offset if k != "dbd" else 0) for k in c.outs_of(o)}
        outs[o] = mine
        view = lambda k: mine[k].view if k in mine else None
        groups.append((ads[o], view("dWu"), view("dWd"), view("dbd")[0] if "dbd" in mine else None))
    L.adapter_bwd_dw(groups, A=c.A)
    torch.cuda.synchronize()
    return outs


def reference(c, segs, keeps=None):
    """fp64 sums over the segments (over the rows that exist, if given) and the sums of magnitudes the bound takes"""
    A = c.A
    ref = dict(dWu=0.0, dWd=0.0, dbd=0.0)
    mag = dict(dWu=0.0, dWd=0.0, dbd=0.0)
    for k, (dy, z, dz, x) in enumerate(segs):
        dy, z, dz, x = dy.double(), z[:, :A].double(), dz[:, :A].double(), x.double()
        if keeps is not None:
            r = torch.tensor(keeps[k], device=DEV)
            dy, z, dz, x = dy[r], z[r], dz[r], x[r]
        ref["dWu"] = ref["dWu"] + dy.t() @ z
        ref["dWd"] = ref["dWd"] + dz.t() @ x
        ref["dbd"] = ref["dbd"] + dz.sum(0, keepdim=True)
        mag["dWu"] = mag["dWu"] + dy.abs().t() @ z.abs()
        mag["dWd"] = mag["dWd"] + dz.abs().t() @ x.abs()
        mag["dbd"] = mag["dbd"] + dz.abs().sum(0, keepdim=True)
    return ref, mag


def seg_index(c, o):
    return sum(c.seg_counts[:o])


def bits_of(outs):
    return {(o, k): v.full.view(torch.int32).clone() for o, d in outs.items() for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", CASES, ids=AC.ids(CASES))
def test_exact(L, case):
    c = case
    ads, pre = make_adapters(c, True, 41), make_prefills(c, True, 42)
    for (dy, z, dz, x) in (s for a in ads for s in a):  # the contract of the operands
        assert not bool(z[:, c.A:].any()) and not bool(dz[:, c.A:].any())
    outs = launch(L, c, ads, pre)
    for o in range(c.adapters):
        s0 = seg_index(c, o)
        keeps = None if c.rows == "all" else [AC.row_keep(c, s0 + k) for k in range(len(ads[o]))]
        ref, _ = reference(c, ads[o], keeps)
        for k, out in outs[o].items():
            assert out.intact(), f"{c.name} adapter {o} {k}: wrote outside its [{out.rows}, {out.cols}]"
            want = pre[o][k].double() + ref[k]
            got = out.view.double()
            if not torch.equal(got, want):
                bad = (got != want) | got.isnan()
                i = bad.nonzero()[0].tolist()
                pytest.fail(f"{c.name} adapter {o} {k}: {int(bad.sum())} of {bad.numel()} elements differ, first at {tuple(i)}: "
                            f"got {got[i[0], i[1]].item()!r} want {want[i[0], i[1]].item()!r}")
    again = bits_of(launch(L, c, ads, pre))
    for key, b in bits_of(outs).items():
        assert torch.equal(b, again[key]), f"{c.name} {key}: two launches differ"


RANDOM = [c for c in CASES if c.random]


@pytest.mark.parametrize("case", RANDOM, ids=AC.ids(RANDOM))
def test_random_within_the_derived_bound(L, case):
    c = case
    ads, pre = make_adapters(c, False, 43), make_prefills(c, False, 44)
    outs = launch(L, c, ads, pre)
    worst = dict(dWu=0.0, dWd=0.0, dbd=0.0)
    fails = []
    for o in range(c.adapters):
        ref, mag = reference(c, ads[o])
        K = len(ads[o]) * c.N
        for k, out in outs[o].items():
            assert out.intact(), f"{c.name} adapter {o} {k}: wrote outside its [{out.rows}, {out.cols}]"
            want = pre[o][k].double() + ref[k]
            bound = 2.0 * K * U * mag[k] + 2.0 * U * want.abs()
            err = (out.view.double() - want).abs()
            bad = ~(err <= bound)
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst[k] = max(worst[k], ratio)
            if bool(bad.any()):
                i = bad.nonzero()[0].tolist()
                fails.append(f"adapter {o} {k}: {int(bad.sum())} bad, first at {tuple(i)}: err {err[i[0], i[1]].item():.3e} "
                             f"bound {bound[i[0], i[1]].item():.3e}")
    print(f"\n[adw] {c.name}: largest err / bound  " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert not fails, f"{c.name}: " + "; ".join(fails)
    again = bits_of(launch(L, c, ads, pre))
    for key, b in bits_of(outs).items():
        assert torch.equal(b, again[key]), f"{c.name} {key}: two launches differ"


@pytest.mark.parametrize("name", ["group_16", "lora_group16"])
def test_group_independence(L, name):
    c = next(x for x in CASES if x.name == name)
    n = c.adapters
    ads, pre = make_adapters(c, False, 45), make_prefills(c, False, 46)
    full = launch(L, c, ads, pre)
    rev = launch(L, c, ads, pre, order=list(range(n - 1, -1, -1)))
    for o in range(n):
        alone = launch(L, c, ads, pre, order=[o])[o]
        five = [(o - o % 5 + j) % n for j in range(5)]  # o sits at position o % 5 of its group of five
        assert five[o % 5] == o
        in_five = launch(L, c, ads, pre, order=five)[o]
        for k, out in alone.items():
            assert out.intact(), (name, o, k)
            for other, what in ((full[o][k], f"in the group of {n} at position {o}"), (rev[o][k], "in the reversed group"),
                                (in_five[k], f"in the group of five {five}")):
                assert other.intact(), (name, o, k, what)
                assert torch.equal(out.view.view(torch.int32), other.view.view(torch.int32)), \
                    f"{name} adapter {o} {k}: launched alone differs from {what}"
