"""GPU: the compact backward -- the backward of a padded forward on the rows that exist -- gives the bits of the padded
backward.  Kernel level: fbl_ln_bwd_rows against fbl_ln_bwd on the padded dout with zero rows, the fused row gather and the
zero-filling scatter against index_select / index_copy_, and the property the design rests on: an NT GEMM gives a row the same
bits whatever other rows it is launched with, on every dispatch route.  Model level: two models from the same parameters and
seed, the route forced off and on, torch.equal on every gradient and on the parameters after three optimizer steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import deberta_oracle as O  # noqa: E402
from tests.golden.make_goldens import _tiny_cfg, synth_batch  # noqa: E402
from tests.test_gpu_model import build, to_dev  # noqa: E402

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
SEED = 0x1234_5678_9ABC


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    return lib


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ------------------------------------------------------------------------------------------------ 1. fbl_ln_bwd_rows
N_PAD = 151  # odd: the last block iteration of the two-rows-per-iteration kernel has a dead slot


def _row_patterns():
    """name -> bool [N_PAD]: the rows that exist"""
    full = torch.ones(N_PAD, dtype=torch.bool)
    end = full.clone(); end[120:] = False                       # a padding run at the very end of the grid
    one = full.clone(); one[77] = False                         # a run of one row
    samples = full.clone()                                      # three samples of 50 rows: the first without padding, runs in the others
    samples[50 + 31:100] = False; samples[100 + 7:150] = False; samples[150] = False  # (and the odd last row dropped: the dead slot's neighbour)
    last = full.clone(); last[:149] = False; last[3] = True     # almost everything dropped, the odd last row kept
    return {"no-padding": full, "run-at-end": end, "run-of-one": one, "samples": samples, "sparse-odd-tail": last}


@pytest.mark.parametrize("H", [1536, 64])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("rowmask", [False, True])
def test_ln_bwd_rows_equals_ln_bwd_on_zero_rows(L, H, p_drop, rowmask):
    """H = 1536: ln_bwd2_kernel (two waves per row); H = 64: ln_bwd_kernel, the one-wave-per-row kernel of an odd H / 64 -- 64 is the
    only such width with an instantiation (fbl_ln_bwd rejects H = 192: tests/test_rowop_cases.py).  Per row pattern: dt and dy at the rows that exist,
    the padded dy at EVERY row, and dgamma / dbeta / dysum, all torch.equal with the padded call (accumulated onto the same
    non-zero start values)."""
    g = _gen(H + int(p_drop * 100))
    t = torch.randn(N_PAD, H, device=DEV, generator=g)
    stats = torch.stack([t.mean(1), 1.0 / (t.var(1, unbiased=False) + 1e-7).sqrt()], 1).contiguous()
    gamma = 1.0 + 0.1 * torch.randn(H, device=DEV, generator=g)
    rm = (torch.rand(N_PAD, device=DEV, generator=g) < 0.8).to(torch.int32) if rowmask else None
    acc0 = torch.randn(3, H, device=DEV, generator=g)
    for name, exist in _row_patterns().items():
        exist = exist.to(DEV)
        sel = torch.nonzero(exist).view(-1)
        Np = sel.numel()
        inv = torch.full((N_PAD,), -1, dtype=torch.int32, device=DEV)
        inv[sel] = torch.arange(Np, dtype=torch.int32, device=DEV)
        dout_c = torch.randn(Np, H, device=DEV, generator=g)
        dout_p = torch.zeros(N_PAD, H, device=DEV).index_copy_(0, sel, dout_c)
        # today's call on the padded rows
        dt_p, dy_p = torch.empty(N_PAD, H, device=DEV), torch.empty(N_PAD, H + 64, dtype=BF16, device=DEV)
        acc_p = acc0.clone()
        L.ln_bwd(dout_p, t, stats, gamma, rowmask=rm, p_drop=p_drop, seed=SEED, out_dt=dt_p, out_dy_bf16=dy_p[:, :H],
                 dgamma=acc_p[0], dbeta=acc_p[1], dysum=acc_p[2], ws=L.ln_bwd_ws(H, DEV))
        # the compact call: outputs poisoned, the [dy | dz] operand's row stride
        dt_c = torch.full((Np, H), float("nan"), device=DEV)
        dy_c = torch.full((Np, H + 64), float("nan"), dtype=BF16, device=DEV)
        dy_pad = torch.full((N_PAD, H), float("nan"), dtype=BF16, device=DEV)
        acc_c = acc0.clone()
        L.ln_bwd_rows(dout_c, inv, t, stats, gamma, rowmask=rm, p_drop=p_drop, seed=SEED, out_dt=dt_c, out_dy_bf16=dy_c[:, :H],
                      out_dy_pad=dy_pad, dgamma=acc_c[0], dbeta=acc_c[1], dysum=acc_c[2], ws=L.ln_bwd_ws(H, DEV))
        assert torch.equal(dt_c, dt_p[sel]), name
        assert torch.equal(dy_c[:, :H], dy_p[sel, :H]), name
        assert bool(dy_c[:, H:].isnan().all()), name  # the columns beside dy are not touched
        assert torch.equal(dy_pad, dy_p[:, :H]), name
        assert float(dy_pad[~exist].abs().max().item() if Np < N_PAD else 0.0) == 0.0, name
        assert torch.equal(acc_c, acc_p), name
        if p_drop > 0:
            assert not torch.equal(dy_c[:, :H].float(), dt_c.to(BF16).float()), "dropout made no difference"


# ------------------------------------------------------------------------------------------------ 2. gather / scatter
@pytest.mark.parametrize("Np", [1, 97, 300])
def test_gather_rows_multi_and_zero_filling_scatter(L, Np):
    """One launch for widths 2 (fp32: 8-byte rows, the 4-byte path), 192, 1536, 4608 and 6144 (bf16), one source with a
    non-contiguous row stride, against index_select; Np = 1 and Np = N.  The scatter against index_copy_ on zeros."""
    N = 300
    g = _gen(Np)
    sel = torch.sort(torch.randperm(N, device=DEV, generator=g)[:Np]).values
    sel32 = sel.to(torch.int32)
    srcs = [torch.randn(N, 2, device=DEV, generator=g)]
    for w in (192, 1536, 4608, 6144):
        srcs.append(torch.randn(N, w, device=DEV, generator=g).to(BF16))
    wide = torch.randn(N + 7, 4608 + 256, device=DEV, generator=g).to(BF16)
    srcs.append(wide[:N, 128:128 + 4608])  # a column block of a wider tensor: row stride != width
    srcs.append(wide[:N, 4:4 + 192])       # ... at an 8-byte offset: copied in 4-byte pieces
    pairs = [(s, torch.full((Np, s.shape[1]), float("nan"), dtype=s.dtype, device=DEV)) for s in srcs]
    L.gather_rows_multi(pairs, sel32)
    for s, d in pairs:
        assert torch.equal(d, s.index_select(0, sel)), tuple(s.shape)
    inv = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    inv[sel] = torch.arange(Np, dtype=torch.int32, device=DEV)
    for (s, d) in pairs[1:6]:
        out = torch.full((N, s.shape[1] + 64), float("nan"), dtype=BF16, device=DEV)
        L.scatter_rows_zero_bf16(d, inv, out[:, :s.shape[1]])
        ref = torch.zeros(N, s.shape[1], dtype=BF16, device=DEV).index_copy_(0, sel, d)
        assert torch.equal(out[:, :s.shape[1]], ref) and bool(out[:, s.shape[1]:].isnan().all())
    # a strided compact source (the dz block of the [dy | dz] operand)
    dyz = torch.randn(Np, 1792, device=DEV, generator=g).to(BF16)
    out = torch.full((N, 192), float("nan"), dtype=BF16, device=DEV)
    L.scatter_rows_zero_bf16(dyz[:, 1536:1728], inv, out)
    assert torch.equal(out, torch.zeros(N, 192, dtype=BF16, device=DEV).index_copy_(0, sel, dyz[:, 1536:1728]))


# ------------------------------------------------------------------------------------------------ 3. GEMM row independence
def _gemm_rows_case(L, M, N, K, sel, seed):
    g = _gen(seed)
    A = torch.randn(M, K, device=DEV, generator=g).to(BF16)
    W = (torch.randn(N, K, device=DEV, generator=g) * 0.05).to(BF16)
    aux = torch.randn(M, N, device=DEV, generator=g).to(BF16)
    for kw_full, kw_sel in (({}, {}), (dict(aux=aux, aux_kind=L.AUX_MUL_BF16), dict(aux=aux[sel].contiguous(), aux_kind=L.AUX_MUL_BF16))):
        full = torch.empty(M, N, dtype=BF16, device=DEV)
        L.gemm(A, W, out_bf16=full, **kw_full)
        part = torch.empty(sel.numel(), N, dtype=BF16, device=DEV)
        L.gemm(A[sel].contiguous(), W, out_bf16=part, **kw_sel)
        assert torch.equal(part, full[sel]), (M, N, K, sel.numel(), bool(kw_full))
        f32 = torch.empty(M, N, dtype=F32, device=DEV)
        L.gemm(A, W, out_f32=f32)
        p32 = torch.empty(sel.numel(), N, dtype=F32, device=DEV)
        L.gemm(A[sel].contiguous(), W, out_f32=p32)
        assert torch.equal(p32, f32[sel]), (M, N, K, sel.numel(), "f32")


def test_gemm_gives_a_row_the_same_bits_on_every_route(L):
    """L.gemm(A[sel], W) == L.gemm(A, W)[sel] bit for bit, with and without a bf16 aux multiply.  M = 4160, N = 2048, K = 256 is
    the smallest shape the 8-phase kernel takes (sixteen 256-row tiles and 64 remainder rows); the selections move rows from
    8-phase tiles into remainder tiles and into 2-stage launches, and back.  M = 300: the 2-stage kernels among themselves."""
    M, N, K = 4160, 2048, 256
    assert L.gemm_plan(M, N, K) == 8
    ar = torch.arange(M, device=DEV)
    # 4100 rows: still the 8-phase kernel, every row behind the first dropped one moves to another tile; the last rows of the
    # full problem (its remainder tile) land inside 256-row tiles
    keep = torch.ones(M, dtype=torch.bool, device=DEV); keep[torch.arange(5, M, 70, device=DEV)[:60]] = False
    sel_a = ar[keep]
    assert L.gemm_plan(sel_a.numel(), N, K) == 8
    _gemm_rows_case(L, M, N, K, sel_a, 1)
    # 8-phase rows into a 2-stage launch (and 200 rows: one partial tile)
    _gemm_rows_case(L, M, N, K, ar[::3].contiguous(), 2)
    _gemm_rows_case(L, M, N, K, ar[4060:4160].contiguous(), 3)  # the remainder tile and the 36 rows in front of it
    # the 2-stage kernels
    ar = torch.arange(300, device=DEV)
    _gemm_rows_case(L, 300, 2048, 256, ar[ar % 5 != 2], 4)
    _gemm_rows_case(L, 300, 192, 1536, ar[7:8], 5)


# ------------------------------------------------------------------------------------------------ 4. the model
def _step_pair(cfg, P, batch, *, expect_compact=True, steps=0):
    """two models from the same parameters and seed in train mode (dropout 0.1 at every site), compact backward forced off and
    on: torch.equal on every trainable gradient and on the video / inputs_embeds gradients after one loss.backward(); with
    `steps`, that many FusedAdam steps on the batch (new dropout masks every step) and torch.equal on the parameters."""
    from frozenbilm_amd.optim import FusedAdam

    res = []
    db = to_dev(batch)
    ids = db.pop("input_ids")
    for force in (False, True):
        m = build(cfg, P, train=True)
        m.compact_backward = force
        v = db["video"].clone().requires_grad_()
        e = dict(m.named_parameters())["deberta.embeddings.word_embeddings.weight"].detach()[ids].clone().requires_grad_()
        out = m(**{**db, "video": v}, inputs_embeds=e)
        out.loss.backward()
        run = out._run
        assert run.bwd_compact == (force and expect_compact), (force, run.bwd_compact)
        if force and expect_compact:
            assert run.pk is None and run.N == ids.numel() + v.shape[0] * v.shape[1] > run.bwd_rows.n  # the forward stayed padded
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad}
        assert len(grads) > 10 and all(bool(torch.isfinite(x).all()) for x in grads.values())
        rec = dict(loss=out.loss.detach().clone(), grads=grads, video=v.grad.clone(), embeds=e.grad.clone())
        if steps:
            opt = FusedAdam(m, lr=1e-3)
            opt.step(clip_max_norm=0.1)
            for _ in range(steps - 1):
                opt.zero_grad()
                o2 = m(**db, input_ids=ids)
                o2.loss.backward()
                assert o2._run.bwd_compact == (force and expect_compact)
                opt.step(clip_max_norm=0.1)
            rec["params"] = {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
        res.append(rec)
    off, on = res
    assert torch.equal(off["loss"], on["loss"])
    for n in off["grads"]:
        assert torch.equal(off["grads"][n], on["grads"][n]), n
    assert torch.equal(off["video"], on["video"]) and torch.equal(off["embeds"], on["embeds"])
    assert float(off["video"].abs().max().item()) > 0 and float(off["embeds"].abs().max().item()) > 0
    for n in off.get("params", {}):
        assert torch.equal(off["params"][n], on["params"][n]), n


@pytest.mark.parametrize("B,Lt,seed", [(5, 90, 3), (2, 33, 4), (7, 130, 5)])
def test_compact_backward_equals_the_padded_backward_tiny(B, Lt, seed):
    """tiny config: 3 layers with the convolution, the enhanced mask decoder, position-table gradients live"""
    cfg = _tiny_cfg()
    P = O.synth_params(cfg, seed=61, std=0.05, ln_jitter=0.1)
    _step_pair(cfg, P, synth_batch(cfg, B=B, L=Lt, seed=seed), steps=3)


def test_compact_backward_stays_off_where_the_padding_rows_take_a_gradient():
    """A batch with no row to drop leaves the route off although it is forced on; so does a backward that is handed a gradient
    on a hidden state (it reaches the padding rows): the gradients are those of the padded backward, bit for bit."""
    cfg = _tiny_cfg()
    P = O.synth_params(cfg, seed=61, std=0.05, ln_jitter=0.1)
    _step_pair(cfg, P, synth_batch(cfg, B=3, L=40, seed=6, ragged=False), expect_compact=False)
    batch = to_dev(synth_batch(cfg, B=4, L=70, seed=13))
    w = torch.randn(4, cfg.max_feats + 70, cfg.hidden_size, device=DEV, generator=_gen(1)) * 1e-2
    grads = []
    for force in (False, True):
        m = build(cfg, P, train=True)
        m.compact_backward = force
        out = m(**batch, output_hidden_states=True)
        (out.loss + (out.hidden_states[2] * w).sum()).backward()
        assert out._run.bwd_rows is None and not out._run.bwd_compact
        grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad})
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n
    # the default rule: a share of dropped rows below the break-even share stays padded
    m = build(cfg, P, train=True)
    b2 = synth_batch(cfg, B=4, L=70, seed=13)
    b2["attention_mask"][:, :] = 1; b2["attention_mask"][0, -2:] = 0  # 2 of 320 rows dropped
    b2["labels"][0, -2:] = -100
    out = m(**to_dev(b2))
    out.loss.backward()
    assert out._run.bwd_rows is None and not out._run.bwd_compact


@pytest.mark.slow
def test_compact_backward_equals_the_padded_backward_at_xlarge_dimensions():
    """the true xlarge dimensions (4 layers, B = 8, L = 256, vocabulary 4096): the 8-phase GEMM tiles, the 192-wide merged
    adapters, the grouped weight-gradient launch and the pooled [dy | dz] operand on the compact layout"""
    cfg = O.OracleConfig()
    cfg.num_hidden_layers, cfg.vocab_size = 4, 4096
    P = O.synth_params(cfg, seed=64, std=0.02, ln_jitter=0.1)
    _step_pair(cfg, P, synth_batch(cfg, B=8, L=256, seed=11))
