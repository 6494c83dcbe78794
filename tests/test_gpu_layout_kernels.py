"""The layout and staging kernels (tests/layout_cases.py) on the MI355X against their definitions, written with torch indexing on
the device.  They move or select values and do no arithmetic, so every check is BIT equality; the two that compute are pinned the
same way: transpose_to_bf16 of fp32 input must be torch's round-to-nearest-even, col2im3 must equal the fp32 sum formed in the
kernel's order ((acc + tap0) + tap1) + tap2 (and fp64 on integers), the D of attn_bwd_prep must equal fbl_attn_rowdot bit for bit
(and fp64 on integers).  fbl_mask_tokens is replayed token by token on the host from the counter-based hash.

Every output lives in a buffer that ends in sentinel elements which must survive (gaps between the matrices of the batched
transpose included); input padding columns, and the rows in front of and behind an input whose neighbours a kernel addresses, hold
the NaN sentinel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import layout_cases as LC
from tests.dropout_replay import fbl_hash
from tests.test_gpu_gemm_routes import BF16, DEV, F32, SENT, Gen, operand

pytestmark = pytest.mark.gpu

I16, I32, I64 = torch.int16, torch.int32, torch.int64
IVIEW = {F32: I32, BF16: I16, I64: I64}
SENTINEL = {F32: SENT[F32], BF16: SENT[BF16], I64: -0x5EA1_DEAD}
G = 192  # sentinel elements behind an output


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


# ------------------------------------------------------------------------------------------------ buffers
class Flat:
    """n elements for the kernel (`v`), G sentinel elements behind them"""

    def __init__(self, n, dtype, fill=None):
        self.n = n
        self.full = torch.empty(n + G, dtype=dtype, device=DEV)
        self.full.view(IVIEW[dtype]).fill_(SENTINEL[dtype])
        self.v = self.full[:n]
        if fill is not None:
            self.v.copy_(fill.reshape(-1))

    def intact(self):
        return bool((self.full.view(IVIEW[self.full.dtype])[self.n:] == SENTINEL[self.full.dtype]).all())

    def bits(self):
        return self.v.view(IVIEW[self.full.dtype])


def between_sentinel_rows(vals, dtype, before=2, after=2):
    """[rows, cols] contiguous view of a buffer with sentinel rows in front of and behind it"""
    rows, cols = vals.shape
    full = torch.empty(before + rows + after, cols, dtype=dtype, device=DEV)
    full.view(IVIEW[dtype]).fill_(SENTINEL[dtype])
    full[before:before + rows] = vals.to(dtype)
    return full[before:before + rows]


def strided_f32(vals, ld):
    full = torch.empty(vals.shape[0], ld, dtype=F32, device=DEV)
    full.view(I32).fill_(SENTINEL[F32])
    full[:, :vals.shape[1]] = vals
    return full[:, :vals.shape[1]]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(IVIEW[a.dtype]), b.contiguous().view(IVIEW[b.dtype]))


def rnd(*shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV)


# ------------------------------------------------------------------------------------------------ transposes
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", LC.TRANSPOSE, ids=LC.ids(LC.TRANSPOSE))
def test_transpose_to_bf16(L, case, dtype):
    c = case
    vals = rnd(c.rows, c.cols, seed=1)
    if dtype == F32 and vals.numel() >= 4:  # ties of the rounding to bf16: to even, down and up
        flat = vals.view(-1)
        flat[0], flat[1], flat[2], flat[3] = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -133
    ld = c.ld_in if c.ld_in is not None else c.cols
    x = strided_f32(vals, ld) if dtype == F32 else operand(vals, ld)
    out = Flat(c.cols * c.rows_pad, BF16)
    L.transpose_to_bf16(x, out.v.view(c.cols, c.rows_pad), rows=c.rows, cols=c.cols)
    torch.cuda.synchronize()
    want = torch.zeros(c.cols, c.rows_pad, dtype=BF16, device=DEV)
    want[:, :c.rows] = x.t().to(BF16)
    assert out.intact(), c.name
    got = out.v.view(c.cols, c.rows_pad)
    assert same_bits(got[:, c.rows:], want[:, c.rows:]), f"{c.name}: padding [{c.rows}, {c.rows_pad}) is not zero"
    assert same_bits(got, want), f"{c.name}: {int((got.view(I16) != want.view(I16)).sum())} elements differ"


@pytest.mark.parametrize("case", LC.TRANSPOSE_BATCHED, ids=LC.ids(LC.TRANSPOSE_BATCHED))
def test_transpose_batched_bf16(L, case):
    c = case
    n = c.rows * c.cols
    sstep, dstep = n + 3 + (n + 3) % 2, n + 7   # source offsets 1, 1 + sstep, ...: all odd; destinations 7 sentinels apart
    src = rnd(1 + c.count * sstep, seed=2).to(BF16)
    soff = [1 + i * sstep for i in range(c.count)]
    doff = [5 + i * dstep for i in range(c.count)]
    assert all(o % 2 == 1 for o in soff)
    dst = Flat(5 + c.count * dstep, BF16)
    want = dst.full.clone()
    for s, d in zip(soff, doff):
        want[d:d + n] = src[s:s + n].view(c.rows, c.cols).t().reshape(-1)
    L.transpose_batched_bf16(src, torch.tensor(soff, dtype=I64, device=DEV), dst.v, torch.tensor(doff, dtype=I64, device=DEV),
                             c.rows, c.cols)
    torch.cuda.synchronize()
    assert same_bits(dst.full, want), f"{c.name}: {int((dst.full.view(I16) != want.view(I16)).sum())} elements differ (gaps included)"


@pytest.mark.parametrize("head_major", [False, True], ids=["bh", "head_major"])
@pytest.mark.parametrize("case", LC.HEAD_T, ids=LC.ids(LC.HEAD_T))
def test_head_transpose(L, case, head_major):
    c = case
    B, S, Sp, nh = c.B, c.S, c.Sp, c.nh
    x = rnd(B * S, 3 * nh * 64, seed=3).to(BF16)
    v = x[:, 2 * nh * 64:]  # the V block of a packed [B*S, 3*nh*64] buffer
    vt = Flat(B * nh * 64 * Sp, BF16)
    L.head_transpose(v, vt.v, B, S, Sp, nh, head_major=head_major)
    torch.cuda.synchronize()
    want = torch.zeros(B, nh, 64, Sp, dtype=BF16, device=DEV)
    want[..., :S] = v.reshape(B, S, nh, 64).permute(0, 2, 3, 1)
    if head_major:
        want = want.permute(1, 2, 0, 3)  # [nh, 64, B, Sp]
    assert vt.intact(), c.name
    assert same_bits(vt.v, want.reshape(-1)), f"{c.name}: {int((vt.bits() != want.reshape(-1).view(I16)).sum())} elements differ"


# ------------------------------------------------------------------------------------------------ attn_bwd_prep, packed rows
@pytest.mark.parametrize("exact", [True, False], ids=["integers", "random"])
@pytest.mark.parametrize("case", LC.PREP, ids=LC.ids(LC.PREP))
def test_attn_bwd_prep_packed_rows(L, case, exact):
    from frozenbilm_amd.model.relpos import rel_index_vector

    c = case
    B, S, Sp, nh, span2 = len(c.lens), c.S, c.Sp, c.nh, c.span2
    H, R = nh * 64, sum(c.lens)
    starts = np.concatenate([[0], np.cumsum(c.lens)]).astype(np.int32)
    row0 = torch.from_numpy(starts).to(DEV)
    g = Gen(51, exact)
    qkv = g.val(R, 3 * H).to(BF16)
    pqk = g.val(span2, 2 * H).to(BF16)
    q, pq, pk = qkv[:, :H], pqk[:, :H], pqk[:, H:]
    dO, O = operand(g.val(R, H), H + 8), operand(g.val(R, H), H + 8)
    relidx = torch.from_numpy(rel_index_vector(S, 256, 512, span2 // 2).copy()).to(DEV)

    def padded(t):  # [B, Sp, cols]: the rows of every sample at positions 0 .. len - 1, zero where the sample has no row
        out = torch.zeros(B, Sp, t.shape[1], dtype=t.dtype, device=DEV)
        for b, n in enumerate(c.lens):
            out[b, :n] = t[starts[b]:starts[b] + n]
        return out

    def run(want_t):
        o = dict(QT=Flat(nh * 64 * B * Sp, BF16) if want_t else None, PQT=Flat(nh * 64 * span2, BF16) if want_t else None,
                 Dv=Flat(B * nh * S, F32), PQX=Flat(nh * 2 * Sp * 64, BF16), PKX=Flat(nh * 2 * Sp * 64, BF16))
        arg = lambda k: o[k].v if o[k] is not None else None
        L.attn_bwd_prep(q, pq, pk, dO, O, arg("QT"), arg("PQT"), arg("Dv"), B, S, Sp, nh, span2, row0=row0, relidx=relidx,
                        PQX=arg("PQX"), PKX=arg("PKX"))
        torch.cuda.synchronize()
        for k, f in o.items():
            assert f is None or f.intact(), k
        return o

    o = run(True)
    want_qt = padded(q).view(B, Sp, nh, 64).permute(2, 3, 0, 1)  # [nh, 64, B, Sp]
    assert same_bits(o["QT"].v, want_qt.reshape(-1)), "QT"
    for b, n in enumerate(c.lens):
        assert not bool(o["QT"].v.view(nh, 64, B, Sp)[:, :, b, n:].view(I16).any()), f"QT columns of sample {b} beyond its {n} rows"
    assert same_bits(o["PQT"].v, pq.reshape(span2, nh, 64).permute(1, 2, 0).reshape(-1)), "PQT"
    t = torch.arange(2 * Sp, device=DEV)
    rows = relidx[(t - Sp + S - 1).clamp(0, 2 * S - 2)].long().clamp(max=span2 - 1)  # the table row of delta = t - Sp
    for k, tab in (("PQX", pq), ("PKX", pk)):
        assert same_bits(o[k].v, tab[rows].reshape(2 * Sp, nh, 64).permute(1, 0, 2).reshape(-1)), k
    # D: positions without a row give zero; bit-equal to fbl_attn_rowdot on the padded grid; exact on integers
    dOp, Op = padded(dO)[:, :S].reshape(B * S, H).contiguous(), padded(O)[:, :S].reshape(B * S, H).contiguous()
    Dv = o["Dv"].v.view(B, nh, S)
    for b, n in enumerate(c.lens):
        assert not bool(Dv[b, :, n:].view(I32).any()), f"D of sample {b} beyond its {n} rows"
    D2 = Flat(B * nh * S, F32)
    L.attn_rowdot(dOp, Op, D2.v, B, S, nh)
    torch.cuda.synchronize()
    assert D2.intact() and same_bits(o["Dv"].v, D2.v), "D differs from fbl_attn_rowdot on the same rows"
    ref = (dOp.double() * Op.double()).view(B, S, nh, 64).sum(-1).permute(0, 2, 1)  # [B, nh, S]
    if exact:
        assert torch.equal(Dv.double(), ref), "D on integers"
    else:  # 64 products, at most 64 additions: the reduction bound of the other tests
        mag = (dOp.double() * Op.double()).abs().view(B, S, nh, 64).sum(-1).permute(0, 2, 1)
        assert bool(((Dv.double() - ref).abs() <= 2 * 64 * 2.0 ** -24 * mag).all())
    # the transposes not requested: the other outputs keep their bits
    o2 = run(False)
    for k in ("Dv", "PQX", "PKX"):
        assert same_bits(o[k].v, o2[k].v), k


# ------------------------------------------------------------------------------------------------ im2col3 / col2im3
def shifted(x3, k):
    """[B, S, C] -> the rows one position before (k = 0), at (1) or after (2) each position, zero beyond the sample"""
    S = x3.shape[1]
    return F.pad(x3, (0, 0, 1, 1))[:, k:k + S]


@pytest.mark.parametrize("case", LC.CONV3, ids=LC.ids(LC.CONV3))
def test_im2col3(L, case):
    B, S, H = case.B, case.S, case.H
    x = between_sentinel_rows(rnd(B * S, H, seed=4), BF16)
    out = Flat(B * S * 3 * H, BF16)
    L.im2col3(x, out.v, B, S, H)
    torch.cuda.synchronize()
    x3 = x.view(B, S, H)
    want = torch.cat([shifted(x3, 0), shifted(x3, 1), shifted(x3, 2)], 2)
    assert out.intact(), case.name
    assert same_bits(out.v, want.reshape(-1)), f"{case.name}: {int((out.bits() != want.reshape(-1).view(I16)).sum())} elements differ"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("exact", [True, False], ids=["integers", "random"])
@pytest.mark.parametrize("case", LC.CONV3, ids=LC.ids(LC.CONV3))
def test_col2im3(L, case, exact, accumulate):
    B, S, H = case.B, case.S, case.H
    g = Gen(61, exact)
    dcol = between_sentinel_rows(g.val(B * S, 3 * H, lo=-8, hi=8) if exact else rnd(B * S, 3 * H, seed=5), F32)
    pre = g.val(B * S, H, lo=-50, hi=50) if exact else rnd(B * S, H, seed=6)
    dx = Flat(B * S * H, F32, pre if accumulate else None)  # accumulate = 0: the sentinel is overwritten, never read
    L.col2im3(dcol, dx.v, B, S, H, accumulate)
    torch.cuda.synchronize()
    taps = dcol.view(B, S, 3, H)
    acc = pre.view(B, S, H).clone() if accumulate else torch.zeros(B, S, H, device=DEV)
    acc64 = acc.double()
    # tap k of output position s - k + 1 reads input position s; a tap whose output position is outside the sample is skipped
    if S > 1:
        acc[:, :S - 1] += taps[:, 1:, 0]
        acc64[:, :S - 1] += taps[:, 1:, 0].double()
    acc += taps[:, :, 1]
    acc64 += taps[:, :, 1].double()
    if S > 1:
        acc[:, 1:] += taps[:, :S - 1, 2]
        acc64[:, 1:] += taps[:, :S - 1, 2].double()
    assert dx.intact(), case.name
    assert same_bits(dx.v, acc.reshape(-1)), f"{case.name}: differs from the fp32 sum in the kernel's order"
    if exact:
        assert torch.equal(dx.v.double(), acc64.reshape(-1)), f"{case.name}: integers"


# ------------------------------------------------------------------------------------------------ embed_gather
@pytest.mark.parametrize("case", LC.EMBED, ids=LC.ids(LC.EMBED))
def test_embed_gather(L, case):
    c = case
    B, T, Lt, H, V = c.B, c.T, c.Lt, c.H, c.V
    gen = torch.Generator().manual_seed(7)
    ids = torch.randint(0, V, (B, Lt), generator=gen)
    ids.view(-1)[0], ids.view(-1)[-1] = 0, V - 1
    ids = ids.to(DEV)
    assert int(ids.min()) == 0 and int(ids.max()) == V - 1
    E = between_sentinel_rows(rnd(V, H, seed=8), F32)
    vproj = between_sentinel_rows(rnd(B * T, H, seed=9), F32) if T else None
    out = Flat(B * (T + Lt) * H, F32)
    L.embed_gather(ids, E, vproj, T, out.v.view(B * (T + Lt), H))
    torch.cuda.synchronize()
    want = E[ids] if not T else torch.cat([vproj.view(B, T, H), E[ids]], 1)
    assert out.intact(), c.name
    assert same_bits(out.v, want.reshape(-1)), c.name


# ------------------------------------------------------------------------------------------------ mask_tokens
VOCAB, MASK_ID, SPECIAL = 30000, 4, (0, 1, 2)


def replay_mask_tokens(ids, p, seed):
    """mask_tokens_kernel on the host: four draws per token keyed by (seed, 4 i + k), compared in float32 like the kernel"""
    n = ids.size
    i4 = np.arange(n, dtype=np.uint64) * np.uint64(4)
    inv = np.float32(2.0 ** -32)
    draw = lambda k: fbl_hash(seed, i4 + np.uint64(k)).astype(np.float32) * inv
    special = np.isin(ids, SPECIAL)
    pick = ~special & (draw(0) < np.float32(p))
    labels = np.where(pick, ids, -100)
    to_mask = pick & (draw(1) < np.float32(0.8))
    to_rand = pick & ~to_mask & (draw(2) < np.float32(0.5))
    rand_id = (fbl_hash(seed, i4 + np.uint64(3)).astype(np.uint64) % np.uint64(VOCAB)).astype(np.int64)
    out = np.where(to_mask, MASK_ID, np.where(to_rand, rand_id, ids))
    return out.astype(np.int64), labels.astype(np.int64), (int(pick.sum()), int(to_mask.sum()), int(to_rand.sum()))


@pytest.mark.parametrize("n", LC.MASK_N)
def test_mask_tokens_replayed(L, n):
    gen = np.random.default_rng(n)
    ids0 = gen.integers(5, VOCAB, size=n).astype(np.int64)
    if n >= 16:  # special ids present: never selected
        ids0[gen.choice(n, size=max(3, n // 8), replace=False)] = gen.choice(SPECIAL, size=max(3, n // 8))
    special = torch.tensor(SPECIAL, dtype=I64, device=DEV)
    seen = [0, 0, 0]
    for p in LC.MASK_P:
        for seed in LC.MASK_SEEDS:
            ids = Flat(n, I64, torch.from_numpy(ids0))
            labels = Flat(n, I64)
            L.mask_tokens(ids.v, labels.v, special, p, MASK_ID, VOCAB, seed)
            torch.cuda.synchronize()
            want_ids, want_labels, counts = replay_mask_tokens(ids0, p, seed)
            assert ids.intact() and labels.intact(), (n, p, seed)
            assert np.array_equal(labels.v.cpu().numpy(), want_labels), (n, p, seed, "labels")
            assert np.array_equal(ids.v.cpu().numpy(), want_ids), (n, p, seed, "ids")
            if p == 0.0:
                assert counts[0] == 0
            if p == 1.0:
                assert counts[0] >= int((~np.isin(ids0, SPECIAL)).sum()) - 1  # (a draw of exactly 1.0f is not below p = 1)
            seen = [a + b for a, b in zip(seen, counts)]
    if n >= 255:
        assert all(s > 0 for s in seen), f"the replay never took one of the three branches: {seen}"
