"""GPU: the LoRA compose kernel (fbl_lora_compose, include/fbl_lora.h) against the float64 reference of tests/lora_cases.py.

Every element must be bf16(x) rounded to nearest even of the float64 value x, except where x lies within the fp32
accumulation bound of a bf16 rounding boundary -- there the value across that boundary passes too (tests/lora_cases.py
derives the bound; tests/test_lora_cases.py shows the reference alone leaves at most 1 % of the elements there).  The
destinations are interior slices of larger guard-filled buffers: the guards keep their bits.  The row-major and the transposed
destination hold identical bits; s = 0 and zero rows of B give exactly bf16(W); the optional fp32 destination holds the value
that was rounded."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lora_cases as LC  # noqa: E402

DEV = "cuda"
GUARD16 = 0x7FC1  # a NaN pattern of bf16, as int16
GUARD32 = -1234.5


def _site(O, I, r, scale, with32, seed=0):
    """one site with all of its operands inside guard-filled buffers; returns (site dict for lib.LoraTable, host inputs,
    the guard-filled buffers)"""
    W, A, B = LC.inputs(O, I, r, seed, scale)
    bigW = torch.full((O + 2, I + 8), GUARD32, dtype=torch.float32, device=DEV)
    bigW[1:1 + O, 4:4 + I] = torch.from_numpy(W)
    big = torch.full((O + 16, I + 16), GUARD16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    bigT = torch.full((I + 16, O + 16), GUARD16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    big32 = torch.full((O + 2, I + 8), GUARD32, dtype=torch.float32, device=DEV) if with32 else None
    site = dict(W=bigW[1:1 + O, 4:4 + I], A=torch.from_numpy(A).to(DEV), B=torch.from_numpy(B).to(DEV), scale=scale,
                dst=big[8:8 + O, 8:8 + I], dstT=bigT[8:8 + I, 8:8 + O], dst32=big32[1:1 + O, 4:4 + I] if with32 else None)
    return site, (W, A, B), (big, bigT, big32)


def _check(site, host, bufs, scale, O, I, r):
    W, A, B = host
    big, bigT, big32 = bufs
    bits = site["dst"].contiguous().view(torch.int16).cpu().numpy()
    bitsT = site["dstT"].contiguous().view(torch.int16).cpu().numpy()
    assert np.array_equal(bits, bitsT.T), "the two layouts differ"
    # guards: everything outside the interior slices keeps its bits
    for buf, (r0, r1, c0, c1) in ((big, (8, 8 + O, 8, 8 + I)), (bigT, (8, 8 + I, 8, 8 + O))):
        g = buf.view(torch.int16).clone()
        g[r0:r1, c0:c1] = GUARD16
        assert bool((g == GUARD16).all()), "a guard element was written"
    x, bound = LC.reference(W, A, B, scale)
    got = LC.bf16_bits_to_f64(bits)
    wrong, n_band = LC.judge(got, x, bound)
    rne = LC.bf16_grid(x)[0]
    print(f"(O, I, r, s) = {(O, I, r, scale)}: {int((got != rne).sum())} of {got.size} elements differ from bf16(float64 value), "
          f"{n_band} lie in the boundary band, {int(wrong.sum())} break the rule")
    assert not wrong.any(), np.argwhere(wrong)[:8]
    w_bits = torch.from_numpy(W).to(torch.bfloat16).view(torch.int16).numpy()
    for row in (3, O - 1):  # zero rows of B: exactly bf16(W)
        assert np.array_equal(bits[row], w_bits[row]), row
    if scale == 0:
        assert np.array_equal(bits, w_bits)
    if big32 is not None:
        v = site["dst32"].contiguous()
        assert np.array_equal(v.to(torch.bfloat16).view(torch.int16).cpu().numpy(), bits), "bf16(dst32) is not dst"
        assert bool((np.abs(v.cpu().numpy().astype(np.float64) - x) <= bound).all())
        g = big32.clone()
        g[1:1 + O, 4:4 + I] = GUARD32
        assert bool((g == GUARD32).all())


@pytest.mark.parametrize("O,I,r", LC.CASES)
@pytest.mark.parametrize("scale,with32", [(LC.SCALE, False), (0.0, True)])
def test_compose_one_site(O, I, r, scale, with32):
    from frozenbilm_amd import lib as L

    site, host, bufs = _site(O, I, r, scale, with32)
    L.lora_compose(L.LoraTable([site], DEV))
    torch.cuda.synchronize()
    _check(site, host, bufs, scale, O, I, r)


def test_compose_sites_of_different_shapes_in_one_launch_and_in_place():
    """the three small cases through ONE table (the grid is sized by the largest site: the others' surplus workgroups leave at
    once), each with an fp32 destination; then W itself as the fp32 destination (model.merge_lora) and a second compose with
    B = 0 on the merged W: the same bf16 bits"""
    from frozenbilm_amd import lib as L

    made = [_site(O, I, r, 0.75, True, seed=7 + n) for n, (O, I, r) in enumerate(LC.CASES[:3])]
    L.lora_compose(L.LoraTable([m[0] for m in made], DEV))
    torch.cuda.synchronize()
    for (site, host, bufs), (O, I, r) in zip(made, LC.CASES[:3]):
        _check(site, host, bufs, 0.75, O, I, r)
    site, host, bufs = made[2]
    before = site["dst"].contiguous().view(torch.int16).clone()
    L.lora_compose(L.LoraTable([dict(site, dst32=site["W"])], DEV))
    site["B"].zero_()
    L.lora_compose(L.LoraTable([dict(site, dst32=None)], DEV))
    torch.cuda.synchronize()
    assert torch.equal(site["dst"].contiguous().view(torch.int16), before)
    assert torch.equal(site["dstT"].contiguous().view(torch.int16), before.t())


def test_binding_refuses_what_the_library_refuses():
    from frozenbilm_amd import lib as L

    site, _, _ = _site(64, 64, 1, 1.0, False)
    bad = dict(site, dst=torch.empty(65, 72, dtype=torch.bfloat16, device=DEV)[1:65, 4:68])  # rows not 16-byte aligned
    with pytest.raises(RuntimeError, match="fbl_lora_compose failed with code -2"):
        L.lora_compose(L.LoraTable([bad], DEV))
