"""GPU: fbl_row_predict (include/fbl_predict.h) against the exact reference of tests/predict_cases.py.

Ids and ranks are selections on identical fp32 inputs: they must match exactly.  Log-probabilities and NLL are compared with
float64 under the bound tests/test_gpu_rowops.py applies to fbl_ce_fwd's row_lse at the same V (C_LSE * 2^-24 * max(|lse|, 1)),
plus the single rounding of the subtraction; with `row_lse` handed in they are `logit - row_lse` bit for bit.  Every case
runs with +inf, NaN and -1e30 in the pad columns V .. ldv-1 and must give identical bits, and twice."""
import pytest
import torch

from tests import predict_cases as PC
from tests.test_gpu_rowops import C_LSE

pytestmark = pytest.mark.gpu

DEV = "cuda"
SWEEP = PC.sweep_cases()


@pytest.fixture(scope="module")
def L():
    from frozenbilm_amd import lib

    lib.load()
    assert torch.cuda.is_available()
    return lib


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def close_or_same_special(what, got, ref, bound):
    """finite reference values within `bound`; where the reference is +-inf or NaN the kernel must say the same"""
    got64 = got.double()
    fin = torch.isfinite(ref)
    special_ok = torch.where(torch.isnan(ref), torch.isnan(got64), got64 == ref)
    assert bool(special_ok[~fin].all()), f"{what}: a non-finite reference value is not reproduced"
    err = (got64 - ref).abs()[fin]
    worst = float((err / bound[fin]).max()) if err.numel() else 0.0
    print(f"[predict] {what}: max err / bound {worst:.3f}")
    assert bool((err <= bound[fin]).all()), f"{what}: {worst:.2f} x the bound"


def run_and_check(L, what, x, V, k, labels):
    """x fp32 [R, V] on the device.  Runs the three pad fills (twice the first), with and without labels / a given lse."""
    R = x.shape[0]
    ld = PC.ru(V, 64)
    ref = PC.ref_predict(x, V, k, labels)
    outs = []
    for fill in (-1e30, float("inf"), float("nan")):
        outs.append(L.row_predict(PC.padded(x, ld, fill), V, k, labels=labels))
    outs.append(L.row_predict(PC.padded(x, ld, -1e30), V, k, labels=labels))
    torch.cuda.synchronize()
    ids, lp, rank, nll = outs[0]
    assert ids.shape == (R, k) and lp.shape == (R, k) and ids.dtype == torch.int32 and lp.dtype == torch.float32
    for other, why in zip(outs[1:], ("+inf in the pad columns", "NaN in the pad columns", "a second run")):
        assert all(same_bits(a, b) for a, b in zip(outs[0], other)), f"{what}: {why} changes the result"
    if R == 0:
        return
    assert torch.equal(ids.long(), ref["ids"]), f"{what}: top-k ids differ from the reference"
    assert torch.equal(rank.long(), ref["rank"]), f"{what}: label ranks differ from the reference"
    lse = ref["lse"]
    close_or_same_special(f"{what} logprob", lp, ref["logprob"], PC.value_bound(C_LSE, lse[:, None], ref["logprob"]).expand_as(lp))
    close_or_same_special(f"{what} nll", nll, ref["nll"], PC.value_bound(C_LSE, lse, ref["nll"]))
    # without labels: the same ids and log-probabilities, no rank / NLL
    ids2, lp2, rank2, nll2 = L.row_predict(PC.padded(x, ld, float("nan")), V, k)
    assert rank2 is None and nll2 is None and same_bits(ids, ids2) and same_bits(lp, lp2), f"{what}: labels change the top-k"
    # a given row_lse is used verbatim: logit - row_lse, bit for bit
    given = torch.logsumexp(x, 1) + 0.125
    ids3, lp3, rank3, nll3 = L.row_predict(PC.padded(x, ld, float("inf")), V, k, labels=labels, row_lse=given)
    torch.cuda.synchronize()
    assert same_bits(ids, ids3) and same_bits(rank, rank3), f"{what}: a given row_lse changes ids / ranks"
    valid = ref["ids"] >= 0
    want = torch.gather(x, 1, ref["ids"].clamp(min=0)) - given[:, None]
    want = torch.where(valid, want, torch.full_like(want, -float("inf")))
    assert torch.equal(torch.nan_to_num(lp3, nan=123.0), torch.nan_to_num(want, nan=123.0)), f"{what}: logprob is not logit - row_lse"
    want_nll = given - torch.gather(x, 1, labels[:, None])[:, 0]
    assert torch.equal(torch.nan_to_num(nll3, nan=123.0), torch.nan_to_num(want_nll, nan=123.0)), f"{what}: nll is not row_lse - logit"


@pytest.mark.parametrize("case", SWEEP, ids=PC.ids(SWEEP))
def test_sweep(L, case):
    c = case
    x, labels = PC.random_rows(c.R, c.V, seed=100 + c.V + c.R, device=DEV)
    if c.R >= 3:
        x[1] = x[1].round()          # many ties
        x[2, : max(1, c.V // 2)] = 1.5
    run_and_check(L, c.name, x, c.V, c.k, labels)


@pytest.mark.parametrize("V,k", [(1000, 5), (1000, 16), (20000, 5), (20000, 16)])
def test_adversarial_rows(L, V, k):
    """V = 1000 has the lane, wave and per-thread-load boundaries of one workgroup, V = 20000 (three chunks, the last partly
    filled) also the boundaries between workgroups and the merge of their candidates"""
    names, x, labels = PC.adversarial_rows(V, k, device=DEV)
    ref = PC.ref_predict(x, V, k, labels)
    ids, _, rank, _ = L.row_predict(PC.padded(x, PC.ru(V, 64), float("nan")), V, k, labels=labels)
    for i, name in enumerate(names):  # (named first, so a failure says which row)
        assert ids[i].tolist() == ref["ids"][i].tolist(), f"V={V} k={k} '{name}': ids"
        assert int(rank[i]) == int(ref["rank"][i]), f"V={V} k={k} '{name}': rank"
    run_and_check(L, f"adversarial V={V} k={k}", x, V, k, labels)


def test_bad_arguments_raise(L):
    x = torch.zeros(2, 64, device=DEV)
    with pytest.raises(ValueError):
        L.row_predict(x, 64, 0)
    with pytest.raises(ValueError):
        L.row_predict(x, 64, 17)
    with pytest.raises(RuntimeError):
        L.row_predict(x, 65, 5)  # V beyond the row
    with pytest.raises(TypeError):
        L.row_predict(x.to(torch.bfloat16), 64, 5)
