"""GPU: the two prompt-tuning kernels (include/fbl_prompt.h) alone.

Shapes: B = 3, L = 7, H in {64, 68} (68: a row that is no multiple of the 128-thread x 16-byte pass, and of no power of two),
T in {0, 2} (without and with video slots), P in {1, 5}.  fbl_embed_assemble copies: its result is EXACTLY the torch
concatenation.  fbl_prompt_grad adds in fp32 in ascending b onto what the buffer holds: its result is EXACTLY the host loop's, and
lies within B . 2^-24 . (|g0| + sum_b |x_b|) of the float64 sum per element (B roundings, each at most half an ulp = 2^-24 relative
to a partial sum that the sum of magnitudes bounds)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, LT, V = 3, 7, 50
CASES = [(H, T, P) for H in (64, 68) for T in (0, 2) for P in (1, 5)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("H,T,P", CASES)
def test_embed_assemble_is_the_concatenation(H, T, P):
    from frozenbilm_amd import lib as L

    g = _gen(H + 10 * T + P)
    S = T + P + LT
    ids = torch.randint(0, V, (B, LT), generator=g).to(DEV)
    E = torch.randn(V, H, generator=g).to(DEV)
    vproj = torch.randn(B * T, H, generator=g).to(DEV) if T else None
    prompt = torch.randn(P, H, generator=g).to(DEV)
    parts = ([vproj.view(B, T, H)] if T else []) + [prompt.expand(B, -1, -1), E[ids]]
    want = torch.cat(parts, 1)
    out = torch.full((B, S, H), 7.5, device=DEV)
    L.embed_assemble(ids, E, vproj, prompt, T, LT, out)
    assert torch.equal(out, want)
    # ids = NULL: the video and prompt rows are written, the text rows keep what they held
    out2 = torch.full((B, S, H), -3.25, device=DEV)
    L.embed_assemble(None, None, vproj, prompt, T, LT, out2)
    assert torch.equal(out2[:, : T + P], want[:, : T + P])
    assert bool((out2[:, T + P:] == -3.25).all())
    # nothing outside [B, S, H] is written: the same call into the middle of a larger sentinel buffer
    big = torch.full((B * S * H + 2 * H,), 9.0, device=DEV)
    L.embed_assemble(ids, E, vproj, prompt, T, LT, big[H: H + B * S * H].view(B, S, H))
    assert bool((big[:H] == 9.0).all()) and bool((big[-H:] == 9.0).all())
    assert torch.equal(big[H: H + B * S * H].view(B, S, H), want)


def _host_sum(g0, dt, first_rows, T, P):
    acc = g0.clone()  # fp32, CPU: plain adds in ascending b
    for r in first_rows:
        acc += dt[r + T: r + T + P]
    return acc


@pytest.mark.parametrize("ragged", [False, True], ids=["grid", "ragged"])
@pytest.mark.parametrize("H,T,P", CASES)
def test_prompt_grad_is_the_ordered_fp32_sum(H, T, P, ragged):
    from frozenbilm_amd import lib as L

    g = _gen(1000 + H + 10 * T + P + ragged)
    S = T + P + LT
    if ragged:  # packed rows: every sample keeps its video and prompt slots and some of its text
        lens = [T + P + n for n in (LT, 0, 3)]
        first = [0, lens[0], lens[0] + lens[1]]
        n_rows = sum(lens)
        row0 = torch.tensor(first + [n_rows], dtype=torch.int32, device=DEV)
    else:
        first, n_rows, row0 = [b * S for b in range(B)], B * S, None
    # magnitudes spread over a few binades, so that the order of the adds shows in the last bits
    dt = torch.randn(n_rows, H, generator=g) * torch.exp2(torch.randint(-6, 7, (n_rows, 1), generator=g).float())
    g0 = torch.randn(P, H, generator=g)
    assert float(g0.abs().min()) > 0
    want = _host_sum(g0, dt, first, T, P)
    reverse = _host_sum(g0, dt, first[::-1], T, P)
    buf = g0.to(DEV)
    L.prompt_grad(dt.to(DEV), row0, B, S, T, buf)
    got = buf.cpu()
    assert torch.equal(got, want)
    if P * H >= 64:
        assert not torch.equal(want, reverse), "the inputs do not tell one order of the adds from another"
    rows = torch.tensor(first)[:, None] + T + torch.arange(P)[None]
    x = dt[rows.reshape(-1)].view(B, P, H).double()
    ref = g0.double() + x.sum(0)
    bound = B * 2.0 ** -24 * (g0.double().abs() + x.abs().sum(0))
    err = (got.double() - ref).abs()
    print(f"[prompt_grad H={H} T={T} P={P} ragged={ragged}] worst error / bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    # a second call accumulates onto the first
    L.prompt_grad(dt.to(DEV), row0, B, S, T, buf)
    assert torch.equal(buf.cpu(), _host_sum(want, dt, first, T, P))
