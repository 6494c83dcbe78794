"""GPU: fine-tuning through the row-selected answer head of the BERT engine (``logit_rows`` under autograd), padded and on
packed rows.  Bounds: the rows route against the full-logits route as on the DeBERTa engine (2e-3 on logits, 1e-4 relative
Frobenius on gradients: same arithmetic, other GEMM tile shapes); packed against padded 1e-5 relative, the bound of
tests/test_gpu_bert_packed.py."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_bert import _params, _to
from tests.test_gpu_bert_packed import CONFIGS, _grads, _mask_rows, _model, _ocfg, _packing_of, _the_batch, _worst_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_ANS = 7


def _setup(name, train=False, p=0.1):
    dims = CONFIGS[name]
    P = _params(_ocfg(dims, n_ans=N_ANS), seed=4)
    b = _the_batch(name, seed=7)
    b.pop("labels")
    B, S = b["input_ids"].shape[0], b["input_ids"].shape[1] + 4
    rows = _mask_rows(name).to(DEV)
    ans = torch.randint(0, N_ANS, (B,), generator=torch.Generator().manual_seed(3)).to(DEV)
    return _model(dims, P, n_ans=N_ANS, p_hid=p, p_att=p, train=train), _to(b), rows, ans, B, S


def _step(m, feed, rows, ans, packed=False, full=False):
    """one forward + cross-entropy on the rows' answer logits + backward; full: the full-logits route, rows read afterwards"""
    m.packed_rows = packed
    m.step_seed = 0  # every step is the same position of the mask stream
    m.zero_grad(set_to_none=True)
    out = m(**feed) if full else m(**feed, logit_rows=rows)
    logits = out.logits.reshape(-1, N_ANS)[rows] if full else out.logits
    F.cross_entropy(logits, ans).backward()
    return out, logits.detach().clone(), _grads(m)


@pytest.mark.parametrize("name", ["small", "multi"])
@pytest.mark.parametrize("train", [False, True])
def test_rows_route_equals_the_full_logits_route(name, train):
    """eval mode, and train mode with hidden and attention dropout live (the head draws none: identical masks)"""
    m, feed, rows, ans, B, S = _setup(name, train=train)
    _, lf, ref = _step(m, feed, rows, ans, full=True)
    out, lr, got = _step(m, feed, rows, ans)
    assert out.loss is None and out.logits.shape == (B, N_ANS) and out.logits.requires_grad
    assert out.__dict__["_run"].pk is None
    assert all(v.norm().item() > 0 for v in ref.values())  # every trainable tensor receives a gradient on both routes
    d_log, worst = (lr - lf).abs().max().item(), _worst_rel(got, ref)
    print(f"[bert rows vs full {name} train={train}] logits max-abs diff {d_log:.3g}, worst relative gradient difference {worst:.3g}")
    assert d_log < 2e-3 and worst < 1e-4
    if train:
        m.eval()
        with torch.no_grad():
            assert (m(**feed, logit_rows=rows).logits - lr).abs().max().item() > 1e-4  # dropout made a difference


@pytest.mark.parametrize("name", ["small", "multi"])
def test_packed_rows_route_equals_the_padded_rows_route(name):
    m, feed, rows, ans, B, S = _setup(name)
    _, lg, ref = _step(m, feed, rows, ans, packed=False)
    out, lp, got = _step(m, feed, rows, ans, packed=True)
    run, have = _packing_of(out, B, S)
    if name == "multi":  # sample 3 has no valid key: the additive mask makes it attend to all S keys, it keeps all S rows
        r0 = run.pk.row0.tolist()
        assert r0[4] - r0[3] == S and r0[3] - r0[2] < S
    assert out.logits.shape == (B, N_ANS) and out.logits.requires_grad
    assert all(v.norm().item() > 0 for v in ref.values())
    r_log, worst = (lp - lg).norm().item() / lg.norm().item(), _worst_rel(got, ref)
    print(f"[bert rows packed vs grid {name}] rows {run.N} of {B * S}: logits relative difference {r_log:.3g}, "
          f"worst relative gradient difference {worst:.3g}")
    assert r_log < 1e-5 and worst < 1e-5


@pytest.mark.parametrize("name", ["small", "multi"])
def test_packed_rows_route_training_step_is_reproducible_and_finite(name):
    m, feed, rows, ans, B, S = _setup(name, train=True)
    a = _step(m, feed, rows, ans, packed=True)
    b = _step(m, feed, rows, ans, packed=True)
    _packing_of(a[0], B, S)
    assert a[0].__dict__["_run"].p_hid > 0 and a[0].__dict__["_run"].p_att > 0
    assert torch.equal(a[1], b[1]) and all(torch.equal(a[2][n], b[2][n]) for n in a[2])
    assert all(torch.isfinite(v).all() for v in a[2].values()) and any(v.abs().max().item() > 0 for v in a[2].values())


@pytest.mark.parametrize("packed", [False, True])
def test_rows_route_edges(packed):
    m, feed, rows, ans, B, S = _setup("small", train=True, p=0.0)

    def one(r, a):
        return _step(m, feed, r, a, packed=packed)[2]

    # several live runs: two forwards, then one backward each; the gradients add up (fixed-order folds everywhere: the only
    # difference to the sum of two separate steps is the fp32 rounding of one more addition per element, ~1e-7 relative)
    rows2, ans2 = rows.flip(0) + 1, ans.flip(0)
    g1, g2 = one(rows, ans), one(rows2, ans2)
    m.zero_grad(set_to_none=True)
    o1, o2 = m(**feed, logit_rows=rows), m(**feed, logit_rows=rows2)
    F.cross_entropy(o1.logits, ans).backward()
    F.cross_entropy(o2.logits, ans2).backward()
    both = _grads(m)
    worst = _worst_rel(both, {n: g1[n] + g2[n] for n in g1})
    print(f"[bert edges packed={packed}] two live runs vs the sum of two steps: worst relative gradient difference {worst:.3g}")
    assert worst < 1e-5
    # R == 0
    empty = m(**feed, logit_rows=torch.zeros(0, dtype=torch.long, device=DEV))
    assert empty.logits.shape == (0, N_ANS) and empty.logits.requires_grad and empty.loss is None
    empty.logits.sum().backward()
    after = _grads(m)
    assert all(torch.equal(after[n], both[n]) for n in both)
    # refused on the host before the step begins
    seed0 = m.step_seed
    for bad in (torch.cat([rows, rows[:1]]), torch.tensor([B * S], device=DEV), torch.tensor([-1], device=DEV)):
        with pytest.raises(ValueError):
            m(**feed, logit_rows=bad)
    labels = torch.full_like(feed["input_ids"], -100)
    labels[:, 1] = 7
    with pytest.raises(RuntimeError):
        m(**feed, logit_rows=rows, labels=labels)
    assert m.step_seed == seed0
    # the no-grad call is as permissive as before, and repeatable bit for bit
    m.eval()
    m.packed_rows = False
    with torch.no_grad():
        dup = torch.cat([rows, rows[:1]])
        a, b = m(**feed, logit_rows=dup).logits, m(**feed, logit_rows=dup).logits
    assert a.shape == (B + 1, N_ANS) and not a.requires_grad and torch.equal(a, b) and torch.equal(a[-1], a[0])
