"""GPU: the two kernels of deep prompt tuning (include/fbl_prompt_layers.h) alone, bit for bit.

Shapes: B in {1, 3}, T in {0, 2} (without and with video slots), P in {1, 5, 128} (one row, a few, FBL_PROMPT_MAX), H in
{4, 64, 1536} (one 16-byte piece per row, less than one 128-thread pass, three passes: the xlarge row), text length 7; the padded
grid b * S and a non-uniform row0 (packed rows: every sample keeps its video and prompt slots and 7, 0 or 3 text rows).  Every
buffer is a view into a larger one with a guard row in front and one behind.

fbl_prompt_rows_write copies: the slot rows hold EXACTLY the parameter's fp32 bits and its round-to-nearest-even bf16 (torch's CPU
cast), every other row keeps its bits.  fbl_prompt_rows_grad adds in fp32 in ascending b onto what g holds: EXACTLY the host
loop's result; then the slot rows of dx are zero and all other rows keep their bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LT = 7
CASES = [pytest.param(B, T, P, H, ragged, id=f"B{B}-T{T}-P{P}-H{H}-{'row0' if ragged else 'grid'}")
         for B in (1, 3) for T in (0, 2) for P in (1, 5, 128) for H in (4, 64, 1536) for ragged in (False, True)]


def _layout(B, T, P, ragged):
    """(first row of every sample, rows, S, row0 tensor or None)"""
    S = T + P + LT
    if ragged:
        lens = [T + P + n for n in (LT, 0, 3)[:B]]
        first = [sum(lens[:b]) for b in range(B)]
        n_rows = sum(lens)
        return first, n_rows, S, torch.tensor(first + [n_rows], dtype=torch.int32, device=DEV)
    return [b * S for b in range(B)], B * S, S, None


def _slot_rows(first, T, P):
    return (torch.tensor(first)[:, None] + T + torch.arange(P)[None]).reshape(-1)


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("B,T,P,H,ragged", CASES)
def test_rows_write_copies_the_parameter_and_touches_nothing_else(B, T, P, H, ragged):
    from frozenbilm_amd import lib as L

    g = torch.Generator().manual_seed(B + 10 * T + 100 * P + H + ragged)
    first, n, S, row0 = _layout(B, T, P, ragged)
    # values over many binades, so that the bf16 rounding meets ties-to-even neighbourhoods, plus exact ties in both directions
    prompt = torch.randn(P, H, generator=g) * torch.exp2(torch.randint(-8, 9, (P, 1), generator=g).float())
    prompt[0, 0], prompt[0, 1] = 1.00390625, 1.01171875  # 1 + 2^-8 -> 1.0 (even), 1 + 3 * 2^-8 -> 1.015625 (even)
    f0 = torch.randn(n + 2, H, generator=g)
    h0 = torch.randn(n + 2, H, generator=g).to(torch.bfloat16)
    slots = _slot_rows(first, T, P) + 1  # (+1: the guard row in front)
    want_f, want_h = f0.clone(), h0.clone()
    want_f[slots] = prompt.repeat(B, 1)
    want_h[slots] = prompt.to(torch.bfloat16).repeat(B, 1)
    pd = prompt.to(DEV)
    f, h = f0.to(DEV), h0.to(DEV)
    L.prompt_rows_write(pd, row0, B, S, T, out_f32=f[1:n + 1], out_bf16=h[1:n + 1])
    assert torch.equal(_bits(f), _bits(want_f)) and torch.equal(_bits(h), _bits(want_h))
    assert torch.equal(_bits(h[slots[0]][:2]), _bits(torch.tensor([1.0, 1.015625]).to(torch.bfloat16)))
    # the rows next to every slot block and the guard rows, spelled out (they are part of the comparison above)
    own = set(slots.tolist())
    for r in first:
        for nb in (r + T, r + T + P + 1):  # buffer rows in front of / behind the block of this sample
            if nb in own:  # (row0 with T = 0 and a sample without text: its neighbour is the next sample's block)
                continue
            assert torch.equal(_bits(f[nb]), _bits(f0[nb])) and torch.equal(_bits(h[nb]), _bits(h0[nb]))
    assert torch.equal(_bits(f[n + 1]), _bits(f0[n + 1])) and torch.equal(_bits(h[n + 1]), _bits(h0[n + 1]))
    # a NULL output is honoured: the other buffer is written, this one is not
    f, h = f0.to(DEV), h0.to(DEV)
    L.prompt_rows_write(pd, row0, B, S, T, out_f32=f[1:n + 1])
    assert torch.equal(_bits(f), _bits(want_f)) and torch.equal(_bits(h), _bits(h0))
    f = f0.to(DEV)
    L.prompt_rows_write(pd, row0, B, S, T, out_bf16=h[1:n + 1])
    assert torch.equal(_bits(f), _bits(f0)) and torch.equal(_bits(h), _bits(want_h))


@pytest.mark.parametrize("B,T,P,H,ragged", CASES)
def test_rows_grad_is_the_ordered_fp32_sum_and_clears_its_rows(B, T, P, H, ragged):
    from frozenbilm_amd import lib as L

    g = torch.Generator().manual_seed(5000 + B + 10 * T + 100 * P + H + ragged)
    first, n, S, row0 = _layout(B, T, P, ragged)
    # magnitudes spread over a few binades, so that the order of the adds shows in the last bits
    dx0 = torch.randn(n + 2, H, generator=g) * torch.exp2(torch.randint(-6, 7, (n + 2, 1), generator=g).float())
    g0 = torch.randn(P, H, generator=g)
    assert float(g0.abs().min()) > 0

    def host(order):
        acc = g0.clone()  # fp32, CPU: plain adds in the given order of the samples
        for r in order:
            acc += dx0[1 + r + T: 1 + r + T + P]
        return acc

    want = host(first)
    if B > 1 and P * H >= 64:
        assert not torch.equal(want, host(first[::-1])), "the inputs do not tell one order of the adds from another"
    slots = _slot_rows(first, T, P) + 1
    want_dx = dx0.clone()
    want_dx[slots] = 0.0
    got = []
    for _ in range(2):  # two identical calls: identical bits
        dx, buf = dx0.to(DEV), g0.to(DEV)
        L.prompt_rows_grad(dx[1:n + 1], row0, B, S, T, P, buf)
        got.append((_bits(buf), _bits(dx)))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert torch.equal(got[0][0], _bits(want))
    assert torch.equal(got[0][1], _bits(want_dx))  # the slot rows are +0.0, every other row (the guards too) keeps its bits
    # g = NULL (a frozen prompt): nothing is summed, the rows are cleared all the same
    dx = dx0.to(DEV)
    L.prompt_rows_grad(dx[1:n + 1], row0, B, S, T, P, None)
    assert torch.equal(_bits(dx), _bits(want_dx))
