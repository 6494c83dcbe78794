"""CPU: the reference of tests/predict_cases.py against brute force on tiny rows; the helpers of predict.Predictions; what
`predict_topk` accepts; the LossLog rule for logged-only extras; `route_for` sends a predict_topk call to the eager route."""
import functools
import math
import types

import pytest
import torch

from frozenbilm_amd import predict as P
from frozenbilm_amd import train_graph as TG
from frozenbilm_amd.loops import LossLog
from tests import predict_cases as PC

INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------ reference vs brute force
def brute(row, k, label):
    """the rule of include/fbl_predict.h, literally, in Python floats"""
    def before(a, b):  # does column a come before column b?
        xa, xb = row[a], row[b]
        if math.isnan(xa) or math.isnan(xb):
            if math.isnan(xa) and math.isnan(xb):
                return a < b
            return math.isnan(xb)
        return xa > xb or (xa == xb and a < b)

    cols = sorted(range(len(row)), key=functools.cmp_to_key(lambda a, b: -1 if before(a, b) else 1))
    ids = (cols + [-1] * k)[:k]
    rank = sum(1 for j, v in enumerate(row) if v > row[label] or (v == row[label] and j < label))
    return ids, rank


TINY = [
    ([1.0, 3.0, 2.0], 1),
    ([2.0, 2.0, 2.0, 2.0], 2),                      # all equal: ascending columns
    ([1.0, 5.0, 5.0, 0.0, 5.0], 4),                 # ties with the label's lower-numbered columns
    ([1.0, 5.0, 5.0, 0.0, 5.0], 1),                 # ... and higher-numbered ones
    ([-INF, 1.0, -INF, -INF], 0),                   # -inf is an ordinary smallest value
    ([-INF, -INF], 1),
    ([NAN, 1.0, -INF, NAN, 0.5], 2),                # NaN below -inf, NaNs ascending by column
    ([NAN, 1.0, -INF, NAN, 0.5], 3),                # a NaN label: nothing compares greater or equal
    ([0.0, -0.0, -1.0], 1),                         # +0 == -0
    ([INF, 1.0, INF], 2),
    ([7.0], 0),
]


@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_reference_matches_brute_force_on_tiny_rows(k):
    for row, label in TINY:
        x = torch.tensor([row], dtype=torch.float32)
        ref = PC.ref_predict(x, len(row), k, labels=torch.tensor([label]))
        ids, rank = brute(row, k, label)
        assert ref["ids"][0].tolist() == ids, (row, k)
        assert int(ref["rank"][0]) == rank, (row, label)
        for slot, c in enumerate(ids):
            got = float(ref["logprob"][0, slot])
            if c < 0:
                assert got == -INF, (row, k, slot)  # k > V: id -1, logprob -inf
            else:
                want = row[c] - float(torch.logsumexp(x.double(), 1))
                assert got == want or (math.isnan(got) and math.isnan(want)), (row, k, slot)


def test_reference_ignores_the_pad_columns_and_takes_a_given_lse():
    x, labels = PC.random_rows(4, 5, seed=3)
    a = PC.ref_predict(PC.padded(x, 64, INF), 5, 3, labels)
    b = PC.ref_predict(PC.padded(x, 64, NAN), 5, 3, labels)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    lse = torch.logsumexp(x, 1)  # fp32
    c = PC.ref_predict(x, 5, 3, labels, lse=lse)
    assert torch.equal(c["logprob"], torch.gather(x.double(), 1, a["ids"]) - lse.double()[:, None])
    assert torch.equal(c["nll"], lse.double() - torch.gather(x.double(), 1, labels[:, None])[:, 0])


def test_case_table_holds_the_shapes_and_boundaries():
    cases = PC.sweep_cases()
    assert {c.V for c in cases} == {1, 2, 5, 63, 64, 65, 257, 1000, 128100}
    assert {c.R for c in cases if c.V != 128100} == {0, 1, 3, 67} and {c.R for c in cases if c.V == 128100} == {3}
    assert {c.k for c in cases} == {1, 5, 16} and any(c.k > c.V for c in cases)
    names, x, labels = PC.adversarial_rows(20000, 5)
    assert len(names) == x.shape[0] == labels.numel() and x.shape[1] == 20000
    for what in PC.BOUNDARIES:
        assert any(what in n for n in names), what
    assert bool(((labels >= 0) & (labels < 20000)).all())


# ------------------------------------------------------------------------------------------------ the output object
def test_predictions_helpers():
    p = P.Predictions(rows=torch.tensor([3, 9, 11, 20]), topk_ids=torch.zeros(4, 5, dtype=torch.int64),
                      topk_logprobs=torch.zeros(4, 5), label_rank=torch.tensor([0, 4, 5, 1]), row_nll=torch.zeros(4))
    assert p.correct().tolist() == [True, False, False, False]
    assert p.correct(5).tolist() == [True, True, False, True]
    assert float(p.accuracy()) == 0.25 and float(p.accuracy(5)) == 0.75 and float(p.count()) == 4.0
    assert p.accuracy().dim() == 0 and not p.accuracy().requires_grad
    e = P.empty(5, "cpu", True)
    assert e.rows.numel() == 0 and e.topk_ids.shape == (0, 5) and e.topk_ids.dtype == torch.int64
    assert float(e.accuracy()) == 0.0 and float(e.accuracy(5)) == 0.0 and float(e.count()) == 0.0  # no NaN for no rows
    unl = P.empty(5, "cpu", False)
    assert unl.label_rank is None and unl.row_nll is None
    with pytest.raises(ValueError):
        unl.correct()


def test_masked_lm_output_carries_predictions_outside_the_tuple():
    from frozenbilm_amd.model.deberta import MaskedLMOutput

    off = MaskedLMOutput(loss=None, logits=torch.zeros(1), hidden_states=None, attentions=None, predictions=None)
    assert off.predictions is None and off["predictions"] is None
    p = P.empty(3, "cpu", False)
    on = MaskedLMOutput(loss=None, logits=torch.zeros(1), hidden_states=None, attentions=None, predictions=p)
    assert on.predictions is p and on["predictions"] is p and on[0] is on["logits"]


# ------------------------------------------------------------------------------------------------ predict_topk
def test_predict_topk_validation_is_pinned():
    """0..16 ints; a bool is refused (True would silently mean "top 1"), and so is anything that is not an int"""
    assert [P.check_topk(v) for v in (0, 1, 5, 16)] == [0, 1, 5, 16]
    for bad in (-1, 17, True, False, 5.0, "5", None):
        with pytest.raises(ValueError):
            P.check_topk(bad)


def test_both_models_have_the_attribute_off_by_default():
    from frozenbilm_amd.model import DebertaV2Config, DebertaV2ForMaskedLM
    from frozenbilm_amd.model.bert import BertConfig, BertForMaskedLM

    cfg = DebertaV2Config(vocab_size=128, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128)
    m = DebertaV2ForMaskedLM(cfg, max_feats=4, features_dim=32)
    assert m.predict_topk == 0 and type(m.predict_topk) is int
    m.predict_topk = 17
    with pytest.raises(ValueError):  # at the call, before the engine is touched
        m(input_ids=torch.zeros(1, 4, dtype=torch.long))
    b = BertForMaskedLM(BertConfig(vocab_size=128, hidden_size=64, num_hidden_layers=1, num_attention_heads=1,
                                   intermediate_size=128, max_position_embeddings=32), max_feats=4, features_dim=32)
    assert b.predict_topk == 0 and type(b.predict_topk) is int


# ------------------------------------------------------------------------------------------------ LossLog extras
class _Run:
    def __init__(self):
        self.logged = []

    def log(self, **scalars):
        self.logged.append(scalars)


def test_losslog_extras_reach_the_meters_only():
    run = _Run()
    log = LossLog(run, "mlm_loss")
    log(torch.tensor(2.0))  # without extras: as before
    assert run.logged == [{"loss": 2.0, "mlm_loss": 2.0}]
    run.logged.clear()
    log(torch.tensor(2.0), {"mlm_acc": torch.tensor(0.25), "mlm_acc5": torch.tensor(0.5), LossLog.WEIGHT: torch.tensor(1.0)})
    assert run.logged == [{"loss": 2.0, "mlm_loss": 2.0}, {"mlm_acc": 0.25, "mlm_acc5": 0.5}]  # not in the loss= sum
    run.logged.clear()
    log.begin(torch.tensor(1.5), {"mlm_acc": torch.tensor(0.5)})  # (a host-side loss: begin reads at once)
    assert run.logged == [{"loss": 1.5, "mlm_loss": 1.5}, {"mlm_acc": 0.5}]


def test_losslog_extras_do_not_trigger_the_nonfinite_stop_and_weight_zero_updates_nothing():
    run = _Run()
    log = LossLog(run, "mlm_loss")
    log(torch.tensor(1.0), {"mlm_acc": torch.tensor(NAN)})  # a non-finite extra is logged, the run goes on
    assert run.logged[0] == {"loss": 1.0, "mlm_loss": 1.0} and math.isnan(run.logged[1]["mlm_acc"])
    run.logged.clear()
    log(torch.tensor(1.0), {"mlm_acc": torch.tensor(0.0), "mlm_acc5": torch.tensor(0.0), LossLog.WEIGHT: torch.tensor(0.0)})
    assert run.logged == [{"loss": 1.0, "mlm_loss": 1.0}]  # a batch without labelled rows updates neither meter
    run.logged.clear()
    # two ranks averaged, one without rows: (0.5 + 0) / 2 over (1 + 0) / 2
    log(torch.tensor(1.0), {"mlm_acc": torch.tensor(0.25), LossLog.WEIGHT: torch.tensor(0.5)})
    assert run.logged[1] == {"mlm_acc": 0.5}
    with pytest.raises(SystemExit):
        log(torch.tensor(NAN), {"mlm_acc": torch.tensor(0.5)})  # the loss itself still stops the run


# ------------------------------------------------------------------------------------------------ graph routes
def test_route_for_sends_a_predict_topk_call_to_the_eager_route():
    def model(**kw):
        return types.SimpleNamespace(inference_graphs=True, training_graphs=True, finetune_graphs=True, packed_rows=False,
                                     decoder_rows=False, n_ans=0, **kw)

    mlm = TG.Call(ids=True, embeds=False, labels=True, rows=None, video_grad=False, mlm=False, hidden_states=False,
                  attentions=False, grad=True)
    ft = mlm._replace(labels=False, rows=3)
    inf = ft._replace(grad=False)
    for call, training, route in ((mlm, True, TG.MLM), (ft, True, TG.FINETUNE), (inf, False, TG.INFERENCE)):
        assert TG.route_for(model(training=training), call) is route                     # no attribute: as before
        assert TG.route_for(model(training=training, predict_topk=0), call) is route     # off: as before
        for k in (1, 5, 16):
            assert TG.route_for(model(training=training, predict_topk=k), call) is None  # on: eager


# ------------------------------------------------------------------------------------------------ the seeds of the model tests
def _fraction_not_separated(x, k=5, sep=2e-3):
    top = x.topk(k + 1, dim=1).values
    return float((~((top[:, :-1] - top[:, 1:]) > sep).all(1)).float().mean())


def test_the_oracles_logits_are_separated_at_the_seeds_of_the_model_tests():
    """tests/test_gpu_predict_model.py compares ids and ranks of two routes exactly where the top six logits of a row are more
    than 2e-3 apart and may leave out 5 % of its rows: at its seeds the CPU oracles leave out none"""
    from oracle import bert_oracle as BO
    from oracle import deberta_oracle as O
    from oracle.model_wrapper import OracleModel
    from tests.golden.make_goldens import _tiny_cfg, synth_batch

    cfg = _tiny_cfg()
    b = synth_batch(cfg, B=5, L=40, seed=31)
    with torch.no_grad():
        lg = OracleModel(cfg, O.synth_params(cfg, seed=74, std=0.2, ln_jitter=0.1)).eval()(**b)["logits"]
    lab = torch.cat([torch.full((5, cfg.max_feats), -100), b["labels"]], 1) != -100
    assert int(lab.sum()) == 21 and _fraction_not_separated(lg[lab]) == 0.0

    small = dict(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128,
                 max_position_embeddings=64)  # SMALL of tests/test_gpu_bert.py, and its _batch()
    bcfg = BO.BertOracleConfig(**small, features_dim=32, max_feats=4, n_ans=0)
    g = torch.Generator().manual_seed(5)
    video = torch.randn(3, 4, 32, generator=g)
    vm = torch.ones(3, 4, dtype=torch.long)
    vm[1, 2:] = 0
    vm[2, 1] = 0
    ids_ = torch.randint(5, 300, (3, 12), generator=g)
    am = torch.ones(3, 12, dtype=torch.long)
    am[0, 9:] = 0
    am[2, 5:] = 0
    ids_[am == 0] = 0
    labels = torch.full((3, 12), -100)
    labels[:, 1::3] = ids_[:, 1::3]
    labels[am == 0] = -100
    with torch.no_grad():
        lg = BO.forward(bcfg, BO.synth_params(bcfg, seed=2, std=0.2, ln_jitter=0.1), ids_, am, video, vm, labels, False)["logits"]
    lab = torch.cat([torch.full((3, 4), -100), labels], 1) != -100
    assert int(lab.sum()) == 9 and _fraction_not_separated(lg[lab]) == 0.0 and _fraction_not_separated(lg[lab], sep=8e-3) == 0.0
